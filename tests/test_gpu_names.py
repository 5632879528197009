"""GPU (MI355X): rfq_decode_names and repaq_amd.tensors.decode_names / decode_tensors(names=True) on the product library - the name lines of an image
and their offsets, in the layout rfq_rows_in takes - against the names of the plain-C oracle's text (tests/_names.py).  The CPU twin is
tests/test_emu_names.py; the hostile images run in a CHILD process here (a device fault ends the process, and the test says so)."""
import json
import os
import subprocess
import sys

import pytest

import _engine as E
import _names as N
import _oracle as O
import _rows as W
import _rows_enc as R
from cases import CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_back_to_default(codec):
    yield
    E.reset_options(codec)


def _oracle_rfq(case):
    try:
        return O.encode_file(case["fq1"], case.get("fq2", b""), case["paired"], case.get("k", 1000) * 1000)
    except O.OracleError:
        return None


DECODABLE = sorted(n for n in CASES if n != "se_name_over_255" and _oracle_rfq(CASES[n]) is not None)


# ---- 1: oracle parity on existing fixtures
@pytest.mark.parametrize("name", DECODABLE)
def test_case_names_like_oracle(codec, name):
    N.check(codec, _oracle_rfq(CASES[name]))


@pytest.mark.parametrize("label", [g[0] for g in W.GENERATED])
def test_generated_names_like_oracle(codec, label):
    assert len(N.check(codec, W.generated(label))) > 100


# ---- 2: small shapes where the writer can go wrong
def test_unparsed_names_at_every_residue_and_beyond_the_tile(codec):
    rfq, names = N.unparsed_names()
    assert N.check(codec, rfq) == names


def test_illumina_names_across_digit_counts(codec):
    rfq, names = N.illumina_digit_counts()
    assert N.check(codec, rfq) == names


def test_coordinates_of_eight_digits_and_more_are_not_storable():
    assert all(e and "cannot be larger than 2M" in e for e in N.coordinates_beyond_the_format())


@pytest.mark.parametrize("shape", [s[0] for s in N.pe_shapes()])
def test_pe_mates_and_name2(codec, shape):
    N.check(codec, dict(N.pe_shapes())[shape])


@pytest.mark.parametrize("shape", [s[0] for s in N.tiny_shapes()])
def test_tiny_shapes(codec, shape):
    N.check(codec, dict(N.tiny_shapes())[shape])


# ---- 3: ranges and walks
@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_ranges_forced_by_slice_bases(codec, walk):
    rfq = W.generated("pe150")
    codec.set_option("RFQ_SLICE_BASES", str(45000))                    # two or three chunks of 20 k bases per range
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    N.check(codec, rfq)
    assert {"walk", "name_lens", "names"} <= set(dict(codec.timings())), codec.timings()
    N.check_size_only(codec, rfq)                                      # (the first of the two passes over the ranges alone)


@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_chunk_index(codec, walk):
    rfq = W.generated("bgi_q40")
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    N.check(codec, rfq, chunk_off=O.chunk_table(rfq))


@pytest.mark.parametrize("step", [700, 5000])
def test_image_slices_concatenate_to_the_whole(codec, step):
    rfq = W.generated("pe150")
    assert N.decode_names_in_slices(codec, rfq, step) == N.expected(rfq)


# ---- 4: size query and refusals
def test_size_query_guarded_buffers_and_refusals(codec):
    N.check_sizes_and_refusals(codec)


def test_empty_image(codec):
    d = codec.dev_put(b"x")
    try:
        r = codec.decode_names(d, 0)
        assert (r.n_rows, r.names_len, r.n_chunks, r.max_name) == (0, 0, 0, 0)
        assert codec.dev_get(r.d_name_off, 8) == b"\0" * 8
    finally:
        codec.dev_free(d)


# ---- 5: the loop closes
def test_rows_and_device_names_reencode_to_the_oracle_image(codec):
    took = [label for label in R.LABELS if N.check_loop(codec, label)]
    assert len(took) >= 3 and {"pe150", "se_var"} <= set(took), took


# ---- 6: hostile images
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import _engine as E, _names as N
from repaq_amd import RfqCodec
c = RfqCodec(device=0, library=E.PRODUCT_LIB)
assert "gfx950" in c.version()
out = {}
for m in [(), (("RFQ_WALK", "exact"),)]:
    out["+".join("%%s=%%s" %% kv for kv in m) or "default"] = N.run_hostile(c, modes=(m,), seed=7, good_every=1, time_bound_s=60.0)
c.close()
print("SUMMARY " + json.dumps(out))
""" % (HERE, os.path.join(HERE, "golden"), os.path.dirname(HERE))


def test_hostile_images_through_names_never_fault_and_leave_no_state():
    r = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, "the child process ended with status %d (negative: a signal - a device fault aborts the process):\n%s" % (r.returncode, tail)
    line = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, tail
    s = json.loads(line[-1][8:])
    for mode, v in s.items():
        assert v["mutants"] >= 500 and v["good_checks"] >= 500 and v["errors"].get("FORMAT", 0) > 50 and v["decoded"] > 50, (mode, v)


# ---- 7: torch - decode, filter on the device, encode
def test_decode_filter_encode_with_tensors(codec):
    """decode_tensors(names=True) on pe150, every third pair kept by a torch mask (name_off rebuilt with cumsum, the blob with a gather), encode_tensors,
    the oracle's decode of that image == the kept records of the original text"""
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import decode_tensors, decode_names, encode_tensors
    rfq = W.generated("pe150")
    text = O.decode_file(rfq, False); lines = text.split(b"\n")[:-1]
    assert all(x == b"+" for x in lines[2::4])
    dev = torch.device("cuda:0")
    img = torch.frombuffer(bytearray(rfq), dtype=torch.uint8).to(dev)
    t = decode_tensors(codec, img, names=True)
    n = t["lens"].numel()
    assert n == len(lines) // 4 and t["name_off"].dtype == torch.int64 and t["name_off"].numel() == n + 1
    blob2, off2 = decode_names(codec, img)
    assert torch.equal(blob2, t["names"]) and torch.equal(off2, t["name_off"])
    assert bytes(t["names"].cpu().numpy().tobytes()) == b"".join(lines[0::4])
    keep = ((torch.arange(n, device=dev) // 2) % 3 == 0)
    off = t["name_off"]; ln = off[1:] - off[:-1]
    new_off = torch.cat([off[:1], ln[keep].cumsum(0)])
    src = torch.repeat_interleave(off[:-1][keep] - new_off[:-1], ln[keep]) + torch.arange(int(new_off[-1]), device=dev)
    codec.clearHeader()
    out = encode_tensors(codec, t["bases"][keep].contiguous(), t["quals"][keep].contiguous(), t["lens"][keep].contiguous(), t["names"][src].contiguous(), new_off,
                         paired=PE_TWO_FILES, chunk_bases=20000)
    got = O.decode_file(bytes(out.cpu().numpy().tobytes()), False)
    want = b"".join(b"\n".join(lines[4 * i:4 * i + 4]) + b"\n" for i in range(n) if (i // 2) % 3 == 0)
    assert got == want and want.count(b"\n") == 4 * int(keep.sum())
