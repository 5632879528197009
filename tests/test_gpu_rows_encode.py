"""GPU (MI355X): rfq_rows_to_text, rfq_encode_rows and repaq_amd.tensors.encode_tensors / rows_to_fastq on the product library - fixed-stride base /
quality rows back to FASTQ text and to .rfq images.  The expected text is each input's own text, the expected image the plain-C oracle's
(tests/_rows_enc.py).  The CPU twin is tests/test_emu_rows_encode.py."""
import pytest

import _engine as E
import _oracle as O
import _rows_enc as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    yield c
    c.close()


def test_enough_plain_cases():
    assert R.N_PLAIN_CASES >= 50 and len(R.INPUTS) == R.N_PLAIN_CASES + 4


@pytest.mark.parametrize("label", R.LABELS)
def test_rows_to_text_equals_the_text(codec, label):
    assert R.check_text_variants(codec, label) >= 4


@pytest.mark.parametrize("label", R.LABELS)
def test_encode_rows_equals_the_oracle_image(codec, label):
    """rfq_encode_rows == the oracle's image; the rows of rfq_decode_rows re-encode to it wherever the image holds the text's reads"""
    assert R.check_image(codec, label) == (label not in R.LOSSY)


def test_records_at_every_residue_across_workgroups(codec):
    R.check_shape(codec, R.residue_set())


def test_one_read_of_70000_bases(codec):
    R.check_shape(codec, R.long_read(), chunk_bases=100000)


def test_no_rows(codec):
    R.check_no_rows(codec)


@pytest.mark.parametrize("label", ["pe150", "se_var", "d6_tiny_pe_interleaved_in"])
def test_size_query_and_caps_one_byte_short(codec, label):
    R.check_sizes_and_short_caps(codec, label)


@pytest.mark.parametrize("label", R.REFUSAL_IDS)
def test_refusal_then_a_good_call(codec, label):
    R.check_refusal(codec, label, through_encoder=False)


@pytest.mark.parametrize("label", ["negative_length", "length_zero", "name_of_no_bytes", "code_5_mid_line", "qual_above_line_end", "name_newline_mid"])
def test_refusal_through_the_encoder(codec, label):
    R.check_refusal(codec, label, through_encoder=True)


def test_argument_refusals(codec):
    R.check_argument_refusals(codec)


@pytest.mark.parametrize("label", ["se_var", "pe150"])
def test_two_row_batches_make_one_file(codec, label):
    R.check_two_batches(codec, label, cut=250 if label == "se_var" else 120)


def test_stage_names(codec):
    R.check_stage_names(codec)


def _names_on_device(t1, t2):
    """the name lines of two texts in HBM, interleaved (R1 of pair k, then its R2), as (blob, offsets): a torch newline index, like test_gpu_rows._text_rows"""
    import torch
    dev = t1.device

    def name_lines(t, base):
        nl = torch.nonzero(t == 10).flatten()
        starts = torch.cat([torch.zeros(1, dtype=nl.dtype, device=dev), nl + 1])
        n = nl.numel() // 4
        return starts[0:4 * n:4] + base, nl[0:4 * n:4] - starts[0:4 * n:4]
    s1, l1 = name_lines(t1, 0); s2, l2 = name_lines(t2, t1.numel())
    start = torch.stack([s1, s2], 1).flatten(); ln = torch.stack([l1, l2], 1).flatten()
    off = torch.zeros(ln.numel() + 1, dtype=torch.int64, device=dev); off[1:] = torch.cumsum(ln, 0)
    row = torch.repeat_interleave(torch.arange(ln.numel(), device=dev), ln)
    src = start[row] + (torch.arange(int(off[-1]), device=dev) - off[row])
    return torch.cat([t1, t2])[src].contiguous(), off


def test_large_pe150_through_encode_tensors():
    """about 2 x 64 MB of PE150: the rows decode_tensors gives for codec.encode's image + the names packed on the device from the text go back through
    encode_tensors to a tensor equal to that image, and through rows_to_fastq to the two input texts"""
    import ctypes as C
    import torch
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import decode_tensors, encode_tensors, rows_to_fastq, pack_names
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    try:
        dev = torch.device("cuda:0")
        a1, a2 = O.gen_np(O.NOVA_PE150, 200_000, seed=23)
        t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
        assert t1.numel() > 60_000_000
        r = c.encode(t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), PE_TWO_FILES, 1_000_000)
        image = torch.empty(r.rfq_len, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        c._check(c._L.rfq_copy_d2d(c._h, C.c_void_p(image.data_ptr()), C.c_void_p(r.d_rfq), r.rfq_len))
        rows = decode_tensors(c, image)
        assert rows["lens"].numel() == 400_000
        blob, off = _names_on_device(t1, t2)
        head = bytes(a1[:int(off[1])].tobytes())
        pb, po = pack_names([head, b"@x"], dev)                                # (pack_names gives the same layout)
        assert bytes(pb.cpu().numpy().tobytes()) == head + b"@x" and po.tolist() == [0, len(head), len(head) + 2] and bytes(blob[:len(head)].cpu().numpy().tobytes()) == head
        c.clearHeader()
        got = encode_tensors(c, rows["bases"], rows["quals"], rows["lens"], blob, off, paired=PE_TWO_FILES, chunk_bases=1_000_000)
        assert got.numel() == image.numel() and torch.equal(got, image)
        f1, f2 = rows_to_fastq(c, rows["bases"], rows["quals"], rows["lens"], blob, off, paired=PE_TWO_FILES)
        assert f1.numel() == t1.numel() and torch.equal(f1, t1) and f2.numel() == t2.numel() and torch.equal(f2, t2)
        wide = decode_tensors(c, image, row_len=151, codes=False, qual_offset=0)                # (byte-granular loads, ASCII, raw qualities)
        g1, g2 = rows_to_fastq(c, wide["bases"], wide["quals"], wide["lens"], blob, off, paired=PE_TWO_FILES, codes=False, qual_offset=0)
        assert torch.equal(g1, t1) and torch.equal(g2, t2)
    finally:
        c.close()
