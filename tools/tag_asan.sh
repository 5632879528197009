#!/bin/bash
# Host-side sanitizer run of rfq_select_rows with a tag (rfq_name_tag): the library's sources as the SIMT-interpreter build (g++, CPU only) and
# tools/tag_asan_main.cpp in ONE stand-alone program under -fsanitize=address,undefined.  The program makes its own rows, names and tags (good shapes and every
# refusal of tests/_tag.py) and checks them against a host loop.  No GPU, no Python in the sanitized process.      tools/tag_asan.sh [WORKDIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
SRC="$ROOT/repaq_amd/csrc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-attributes -I"$ROOT/tests/emu/include" \
    -x c++ "$SRC/rfq_api.hip" "$SRC/rfq_encode.hip" "$SRC/rfq_decode.hip" "$ROOT/tools/tag_asan_main.cpp" -o "$WORK/tag_asan" -lpthread
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$WORK/tag_asan"
