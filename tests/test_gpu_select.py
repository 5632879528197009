"""GPU (MI355X): rfq_select_rows and repaq_amd.tensors.select_rows on the product library - rows to the kept rows, trimmed to a window each, with their
lengths, names and name offsets - against numpy on the host (tests/_select.py).  The CPU twin is tests/test_emu_select.py."""
import random

import numpy as np
import pytest

import _engine as E
import _oracle as O
import _rows_enc as R
import _select as S

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


# ---- 1: identity
@pytest.mark.parametrize("label", [g[0] for g in S.W.GENERATED])
def test_everything_kept_is_the_input(codec, label):
    S.check_identity(codec, label)


# ---- 2: windows at every residue, buffers at shifts 0 / 1 / 7 / 15
@pytest.mark.parametrize("row_len_in", S.WINDOW_ROW_LENS)
def test_windows_at_every_residue(codec, row_len_in):
    S.check_windows(codec, row_len_in)


# ---- 3: masks
@pytest.mark.parametrize("n_rows", S.MASK_ROWS)
def test_mask_patterns(codec, n_rows):
    S.check_masks(codec, n_rows)


# ---- 4: both forms of the scan
@pytest.mark.parametrize("n_rows", [16384, 16385, 40001])
def test_scan_small_and_tiled(codec, n_rows):
    S.check_scan(codec, n_rows)


# ---- 5: pairs and min_len
def test_pairs_and_min_len(codec):
    S.check_pairs_and_min_len(codec)


# ---- 6: names
def test_names_at_every_residue(codec):
    S.check_name_residues(codec)


def test_name_longer_than_a_tile(codec):
    S.check_long_name(codec)


def test_rows_without_names_and_each_output_alone(codec):
    S.check_no_names_and_each_output_alone(codec)


# ---- 7: sizes and refusals
def test_caps_one_short(codec):
    S.check_short_caps(codec)


@pytest.mark.parametrize("label", S.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    S.check_device_refusal(codec, label)


def test_refused_on_the_host(codec):
    S.check_host_refusals(codec)


# ---- 8: closing the square
@pytest.mark.parametrize("label", R.LABELS)
def test_text_rows_select_back_to_text_and_to_the_oracle_image(codec, label):
    S.check_square(codec, label)


# ---- 9: twice is the same
@pytest.mark.parametrize("label", [g[0] for g in S.W.GENERATED])
def test_twice_is_the_same(codec, label):
    S.check_square(codec, label, twice=True)


# ---- 10: torch - fastq, select on the device, encode
@pytest.mark.parametrize("side_stream", [False, True])
def test_select_rows_with_tensors(codec, side_stream):
    """the PE150 trimmed-pair input of test_gpu_text_rows.test_fastq_filter_encode_with_tensors: tensors.select_rows(keep=lens >= 100, pairs=True) gives the
    tensors of the torch recipe it replaces, encode_tensors of them the oracle's image of the filtered text; a second call trims the kept rows"""
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, encode_tensors, select_rows
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
        assert t["lens"].numel() == 600 and t["bases"].shape == (600, 150)
        s = select_rows(codec, t, keep=t["lens"] >= 100, pairs=True)
        # the recipe it replaces
        keep = (t["lens"].view(-1, 2) >= 100).all(dim=1).repeat_interleave(2)
        off = t["name_off"]; ln = off[1:] - off[:-1]
        new_off = torch.cat([off[:1], ln[keep].cumsum(0)])
        src = torch.repeat_interleave(off[:-1][keep] - new_off[:-1], ln[keep]) + torch.arange(int(new_off[-1]), device=dev)
        want = {"bases": t["bases"][keep], "quals": t["quals"][keep], "lens": t["lens"][keep], "names": t["names"][src], "name_off": new_off}
        for k, w in want.items():
            assert s[k].dtype == w.dtype and torch.equal(s[k], w), k
        codec.clearHeader()
        out = encode_tensors(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, chunk_bases=20000)
        u = select_rows(codec, s, start=torch.full_like(s["lens"], 5), length=s["lens"] - 10, pairs=True)
    stream.synchronize()
    kept = [k for k in range(300) if len(l1[4 * k + 1]) >= 100 and len(l2[4 * k + 1]) >= 100]
    assert 0 < len(kept) < 300 and int(s["lens"].numel()) == 2 * len(kept)
    masked = sum(1 for k in range(300) for l in (l1, l2) if len(l[4 * k + 1]) < 100)
    assert s["dropped"] == {"mask": masked, "short": 0, "mate": 600 - 2 * len(kept) - masked}
    w1 = b"".join(b"\n".join(l1[4 * k:4 * k + 4]) + b"\n" for k in kept); w2 = b"".join(b"\n".join(l2[4 * k:4 * k + 4]) + b"\n" for k in kept)
    assert bytes(out.cpu().numpy().tobytes()) == O.encode_file(w1, w2, O.PE_TWO_FILES, 20000)
    # the second call: bases [5, len - 5) of every kept row, padded to the longest window
    sb, sq, sl = s["bases"].cpu().numpy(), s["quals"].cpu().numpy(), s["lens"].cpu().numpy()
    L = int(sl.max()) - 10
    wb = np.full((len(sl), L), 255, np.uint8); wq = np.full((len(sl), L), 255, np.uint8)
    for i, n in enumerate(sl):
        wb[i, :n - 10] = sb[i, 5:n - 5]; wq[i, :n - 10] = sq[i, 5:n - 5]
    assert u["bases"].shape == (len(sl), L) and np.array_equal(u["bases"].cpu().numpy(), wb) and np.array_equal(u["quals"].cpu().numpy(), wq)
    assert np.array_equal(u["lens"].cpu().numpy(), sl - 10) and torch.equal(u["names"], s["names"]) and torch.equal(u["name_off"], s["name_off"])
    assert u["dropped"] == {"mask": 0, "short": 0, "mate": 0}
