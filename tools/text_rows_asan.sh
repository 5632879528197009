#!/bin/bash
# Host-side sanitizer run of rfq_text_rows: the library's sources as the SIMT-interpreter build (g++, CPU only) and tools/text_rows_asan_main.cpp in ONE
# stand-alone program under -fsanitize=address,undefined, on the fixture texts written by tests/_text_rows.py (write_fixtures: good inputs and junk).
# No GPU, no Python in the sanitized process.      tools/text_rows_asan.sh [WORKDIR]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
WORK="${1:-$(mktemp -d)}"
mkdir -p "$WORK"
(cd "$ROOT/tests" && python -c "import sys; sys.path[:0] = ['.', 'golden', '..']; import _text_rows; print(*_text_rows.write_fixtures(sys.argv[1]))" "$WORK")
SRC="$ROOT/repaq_amd/csrc"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Wno-attributes -I"$ROOT/tests/emu/include" \
    -x c++ "$SRC/rfq_api.hip" "$SRC/rfq_encode.hip" "$SRC/rfq_decode.hip" "$ROOT/tools/text_rows_asan_main.cpp" -o "$WORK/text_rows_asan" -lpthread
UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$WORK/text_rows_asan" "$WORK"/*.fq
