"""The decode path's range plan (repaq_amd/csrc/dec/ranges.h: the cut rule, the queue with its halving, bug_compat's pieces), driven directly through
tests/ranges_main.cpp over synthetic chunk tables - the halving branch otherwise needs 4 GiB of text per output.  Plain g++, no library, no GPU; once more
under the address and undefined-behaviour sanitizers (a stand-alone program)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "repaq_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]], ids=["plain", "asan_ubsan"])
def test_range_plan(tmp_path, flags):
    exe = str(tmp_path / "ranges_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-I" + CSRC, os.path.join(HERE, "ranges_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("RANGES_OK") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
