"""GPU (MI355X): rfq_text_rows and repaq_amd.tensors.fastq_to_tensors on the product library - FASTQ text to per-read base / quality rows, lengths and
names - against the text's own lines or the plain-C oracle's round trip (tests/_text_rows.py).  The CPU twin is tests/test_emu_text_rows.py; the junk
texts run in a CHILD process here (a device fault ends the process, and the test says so)."""
import json
import os
import subprocess
import sys

import pytest

import _engine as E
import _oracle as O
import _rows_enc as R
import _text_rows as T

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


# ---- 1: every golden case
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_case_rows_and_names(codec, name):
    assert T.check_case(codec, name) == T.ROUTES[name]


# ---- 2: generated inputs over the row variants, text at shifts 1 / 7 / 15
@pytest.mark.parametrize("label", T.GEN_LABELS)
def test_generated_over_variants(codec, label):
    T.check_generated(codec, label)


# ---- 3: small shapes
def test_read_lengths_and_names_at_every_residue(codec):
    T.check_shapes(codec)


def test_one_record_with_and_without_final_newline(codec):
    T.check_one_record_and_final(codec)


def test_long_read_and_pad_fill(codec):
    T.check_long_read_and_pad(codec)


def test_each_output_alone(codec):
    T.check_each_output_alone(codec)


# ---- 4: pairs
def test_pairs_two_files_and_interleaved(codec):
    T.check_pairs(codec)


# ---- 5: streaming
@pytest.mark.parametrize("step", [997, 20011])
def test_text_fed_in_steps_equals_one_shot(codec, step):
    T.check_streaming(codec, step)


def test_forced_slices_consume_less_and_the_loop_equals_one_shot(codec):
    T.check_streaming_forced_slices(codec)


# ---- 6: sizes and refusals
def test_caps_one_short(codec):
    T.check_short_caps(codec)


def test_quality_line_one_short_and_one_long(codec):
    T.check_quality_lengths(codec)


def test_argument_refusals(codec):
    T.check_argument_refusals(codec)


def test_empty_text(codec):
    T.check_empty_text(codec)


# ---- 7: closing the square
@pytest.mark.parametrize("label", R.LABELS)
def test_text_rows_back_to_text_and_to_the_oracle_image(codec, label):
    T.check_square(codec, label)


# ---- 8: junk that is still input, once, in a child process
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import _engine as E, _text_rows as T
from repaq_amd import RfqCodec
c = RfqCodec(device=0, library=E.PRODUCT_LIB)
assert "gfx950" in c.version()
out = T.run_junk(c)
c.close()
print("SUMMARY " + json.dumps(out))
""" % (HERE, os.path.join(HERE, "golden"), os.path.dirname(HERE))


def test_junk_returns_rows_or_a_code_and_leaves_no_state():
    r = subprocess.run([sys.executable, "-c", CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, "the child process ended with status %d (negative: a signal - a device fault aborts the process):\n%s" % (r.returncode, tail)
    line = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, tail
    s = json.loads(line[-1][8:])
    assert s["calls"] == 72 and s["rows"] > 0 and s["errors"], s


# ---- 9: torch - fastq, filter on the device, encode
@pytest.mark.parametrize("side_stream", [False, True])
def test_fastq_filter_encode_with_tensors(codec, side_stream):
    """fastq_to_tensors on a PE150 pair whose reads were trimmed to several lengths, pairs with both mates >= 100 bases kept by a torch mask (the
    module docstring's recipe), encode_tensors: the image equals the oracle's image of the filtered text"""
    import random
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, encode_tensors
    rng = random.Random(31)
    fq1, fq2 = O.gen(O.NOVA_PE150, 300, seed=41)

    def trim(text):
        ln = text.split(b"\n")[:-1]
        for i in range(0, len(ln), 4):
            k = rng.choice((150, 150, 120, 99, 60))
            ln[i + 1] = ln[i + 1][:k]; ln[i + 3] = ln[i + 3][:k]
        return b"\n".join(ln) + b"\n", ln
    fq1, l1 = trim(fq1); fq2, l2 = trim(fq2)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(fq1), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(fq2), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES)
        n = t["lens"].numel()
        assert n == 600 and t["consumed"] == (len(fq1), len(fq2)) and t["bases"].shape == (600, 150)
        keep = (t["lens"].view(-1, 2) >= 100).all(dim=1).repeat_interleave(2)
        off = t["name_off"]; ln = off[1:] - off[:-1]
        new_off = torch.cat([off[:1], ln[keep].cumsum(0)])
        src = torch.repeat_interleave(off[:-1][keep] - new_off[:-1], ln[keep]) + torch.arange(int(new_off[-1]), device=dev)
        codec.clearHeader()
        out = encode_tensors(codec, t["bases"][keep].contiguous(), t["quals"][keep].contiguous(), t["lens"][keep].contiguous(), t["names"][src].contiguous(), new_off,
                             paired=PE_TWO_FILES, chunk_bases=20000)
    stream.synchronize()
    kept = [k for k in range(300) if len(l1[4 * k + 1]) >= 100 and len(l2[4 * k + 1]) >= 100]
    assert 30 < len(kept) < 300 and int(keep.sum()) == 2 * len(kept)
    w1 = b"".join(b"\n".join(l1[4 * k:4 * k + 4]) + b"\n" for k in kept); w2 = b"".join(b"\n".join(l2[4 * k:4 * k + 4]) + b"\n" for k in kept)
    assert bytes(out.cpu().numpy().tobytes()) == O.encode_file(w1, w2, O.PE_TWO_FILES, 20000)
