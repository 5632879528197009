"""GPU (MI355X): hostile .rfq images (tests/_hostile.py) through rfq_decode_rows - every call returns one of _hostile.ALLOWED or rows within the time
bound, and the same context then decodes the good image to the right rows.  In a CHILD process, like tests/test_gpu_hostile.py: a device fault ends
the process, and the test says so."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import _engine as E, _rows as W
from repaq_amd import RfqCodec
c = RfqCodec(device=0, library=E.PRODUCT_LIB)
assert "gfx950" in c.version()
out = {}
for m in [(), (("RFQ_WALK", "exact"),)]:
    out["+".join("%%s=%%s" %% kv for kv in m) or "default"] = W.run_hostile(c, modes=(m,), seed=7, good_every=1, time_bound_s=60.0)
c.close()
print("SUMMARY " + json.dumps(out))
""" % (HERE, os.path.join(HERE, "golden"), os.path.dirname(HERE))


def test_hostile_images_through_rows_never_fault_and_leave_no_state():
    r = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, "the child process ended with status %d (negative: a signal - a device fault aborts the process):\n%s" % (r.returncode, tail)
    line = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, tail
    s = json.loads(line[-1][8:])
    for mode, v in s.items():
        assert v["mutants"] >= 500 and v["good_checks"] >= 500 and v["errors"].get("FORMAT", 0) > 50 and v["decoded"] > 50, (mode, v)
