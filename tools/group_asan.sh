#!/bin/bash
# Host-side sanitizer run of rfq_group_rows: the library's sources as the SIMT-interpreter build (g++, CPU only) and tools/group_asan_main.cpp in ONE stand-alone
# program under -fsanitize=address,undefined.  The program makes its own rows and bins (good shapes and every refusal of tests/_group.py) and checks them against
# a host loop.  No GPU, no Python in the sanitized process.      tools/group_asan.sh [WORKDIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
SRC="$ROOT/repaq_amd/csrc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-attributes -I"$ROOT/tests/emu/include" \
    -x c++ "$SRC/rfq_api.hip" "$SRC/rfq_encode.hip" "$SRC/rfq_decode.hip" "$ROOT/tools/group_asan_main.cpp" -o "$WORK/group_asan" -lpthread
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$WORK/group_asan"
