#!/bin/bash
# Host-side sanitizer run of rfq_kmers_init, rfq_kmers_rows and rfq_kmers_read: the library's sources as the SIMT-interpreter build (g++, CPU only) and
# tools/kmers_asan_main.cpp in ONE stand-alone program under -fsanitize=address,undefined.  The program makes its own rows and tables (the good shapes and every
# refusal of tests/_kmers.py) and checks them against a host reference.  No GPU, no Python in the sanitized process.      tools/kmers_asan.sh [WORKDIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
SRC="$ROOT/repaq_amd/csrc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-attributes -I"$ROOT/tests/emu/include" \
    -x c++ "$SRC/rfq_api.hip" "$SRC/rfq_encode.hip" "$SRC/rfq_decode.hip" "$ROOT/tools/kmers_asan_main.cpp" -o "$WORK/kmers_asan" -lpthread
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$WORK/kmers_asan"
