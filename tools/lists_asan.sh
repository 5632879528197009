#!/bin/bash
# Host-side sanitizer run of the fused decode's position-list passes: the library's sources as the SIMT-interpreter build (g++, CPU only) and
# tools/lists_asan_main.cpp in ONE stand-alone program under -fsanitize=address,undefined, on the fixture images written by tests/_lists.py (write_fixtures),
# each in a heap allocation that ends with the image's last byte, whole and cut 1 .. 19 bytes short.  No GPU, no Python in the sanitized process.
#     tools/lists_asan.sh [WORKDIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
(cd "$ROOT/tests" && python -c "import sys; sys.path[:0] = ['.', 'golden', '..']; import _lists; print(len(_lists.write_fixtures(sys.argv[1])), 'images')" "$WORK")
SRC="$ROOT/repaq_amd/csrc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-attributes -I"$ROOT/tests/emu/include" \
    -x c++ "$SRC/rfq_api.hip" "$SRC/rfq_encode.hip" "$SRC/rfq_decode.hip" "$ROOT/tools/lists_asan_main.cpp" -o "$WORK/lists_asan" -lpthread
# (detect_leaks=0: the interpreter's streams are null pointers, so the context takes its second stream for missing and makes its events again on every call -
# eight bytes each, in the interpreter build alone)
ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$WORK/lists_asan" "$WORK"/*.rfq
