"""GPU (MI355X): rfq_decode_rows and repaq_amd.tensors.decode_tensors on the product library - the reads of an image as fixed-stride base /
quality rows - against rows built from the plain-C oracle's text (tests/_rows.py) and from rfq_decode_batch's own text, which the rest of
the suite pins to the reference."""
import numpy as np
import pytest

import _engine as E
import _oracle as O
import _rows as W
from cases import CASES
from repaq_amd import RfqError

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


@pytest.mark.parametrize("codes", [False, True], ids=["ascii", "codes"])
@pytest.mark.parametrize("name", DECODABLE)
def test_case_rows_like_oracle(codec, name, codes):
    W.check(codec, _oracle_rfq(CASES[name]), codes=codes)


@pytest.mark.parametrize("label", [g[0] for g in W.GENERATED])
def test_generated_rows_like_oracle(codec, label):
    assert W.check(codec, W.generated(label), codes=True) > 100


@pytest.mark.parametrize("qual_offset,extra,codes", [(0, 0, False), (33, 1, True), (64, 1, False), (33, "x16", True), (0, "x16", False)])
@pytest.mark.parametrize("label", ["pe150", "se_var"])
def test_row_len_and_offset_variants(codec, label, qual_offset, extra, codes):
    rfq = W.generated(label)
    ml = codec.decode_rows_bytes(rfq, bases=False, quals=False, lens=False)[1]
    L = (ml // 16 + 1) * 16 if extra == "x16" else ml + extra
    W.check(codec, rfq, row_len=L, codes=codes, qual_offset=qual_offset, pad_base=7, pad_qual=0)


@pytest.mark.parametrize("name", sorted(E.rle_goldens()))
def test_legacy_run_length_quality_images(codec, name):
    W.check(codec, bytes.fromhex(E.rle_goldens()[name]["rfq_hex"]), codes=True)


def test_size_query_equals_the_decode_on_every_walk_path(codec):
    rfq = W.generated("se_var"); offs = O.chunk_table(rfq)
    n, ml, _, _, _ = W.expected(rfq)
    d = codec.dev_put(rfq)
    try:
        for opts, index in (({}, None), ({"RFQ_WALK": "exact"}, None), ({}, offs), ({"RFQ_WALK": "exact"}, offs), ({"RFQ_GW_SHIFT": "12"}, None)):
            for k, v in opts.items():
                codec.set_option(k, v)
            q = codec.decode_rows(d, len(rfq), chunk_off=index)
            assert (q.n_rows, q.max_len, q.n_chunks, q.consumed) == (n, ml, len(offs) - 1, len(rfq)), (opts, index is not None)
            E.reset_options(codec)
    finally:
        codec.dev_free(d)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "misaligned"])
def test_refusals_write_nothing_and_leave_the_context_usable(codec, shift):
    rfq = W.generated("pe150")
    n, ml, B, Q, lens = W.expected(rfq, row_len=160)
    d = codec.dev_put(rfq)
    gb, gq, gl = W.Guarded(codec, n * 160, shift=shift), W.Guarded(codec, n * 160, shift=shift), W.Guarded(codec, 4 * n, shift=4 * shift)
    try:
        before = (gb.body(), gq.body(), gl.body())
        full = dict(d_bases=gb.ptr, bases_cap=n * 160, d_quals=gq.ptr, quals_cap=n * 160, d_lens=gl.ptr, lens_cap=n)
        for what, kw in (("row_len < max_len", dict(full, row_len=ml - 1, bases_cap=n * (ml - 1), quals_cap=n * (ml - 1))),
                         ("bases one row short", dict(full, row_len=160, bases_cap=n * 160 - 160)),
                         ("quals one byte short", dict(full, row_len=160, quals_cap=n * 160 - 1)),
                         ("lens one entry short", dict(full, row_len=160, lens_cap=n - 1))):
            with pytest.raises(RfqError) as ei:
                codec.decode_rows(d, len(rfq), **kw)
            assert ei.value.code == -8, (what, ei.value)
            assert (gb.body(), gq.body(), gl.body()) == before, what
        r = codec.decode_rows(d, len(rfq), row_len=160, **full)
        assert r.n_rows == n
        assert np.array_equal(np.frombuffer(gb.body(), np.uint8).reshape(n, 160), B)
        assert np.array_equal(np.frombuffer(gq.body(), np.uint8).reshape(n, 160), Q)
        assert np.array_equal(np.frombuffer(gl.body(), np.int32), lens)
        assert gb.guards_intact() and gq.guards_intact() and gl.guards_intact()
    finally:
        codec.dev_free(d)
        for g in (gb, gq, gl):
            g.free()


@pytest.mark.parametrize("opts", [{"RFQ_SLICE_BASES": "45000"}, {"RFQ_SLICE_BASES": "45000", "RFQ_WALK": "exact"}, {"RFQ_WALK": "exact"},
                                  {"RFQ_MATERIALISE": "1"}, {"RFQ_STREAMS": "1"}], ids=["slices", "slices_exact", "exact", "materialise", "one_stream"])
def test_formulations(codec, opts):
    rfq = W.generated("pe150")
    for k, v in opts.items():
        codec.set_option(k, v)
    W.check(codec, rfq, row_len=160, codes=True)
    W.check(codec, W.generated("bgi_q40"), codes=False, chunk_off=O.chunk_table(W.generated("bgi_q40")))


@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_ranges_with_one_output_left_out(codec, walk):
    rfq = W.generated("pe150")
    codec.set_option("RFQ_SLICE_BASES", str(45000))                    # two or three chunks of 20 k bases per range
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    n, ml, B, Q, lens = W.expected(rfq, row_len=160, codes=True)
    for which in ("bases", "quals", "lens"):
        gn, gml, gb, gq, gl = codec.decode_rows_bytes(rfq, row_len=160, codes=True, **{which: False})
        assert (gn, gml) == (n, ml)
        for name, got, want in (("bases", gb, B), ("quals", gq, Q), ("lens", gl, lens)):
            assert (got is None) if name == which else np.array_equal(got, want), (which, name)


@pytest.mark.parametrize("step", [700, 5000])
def test_image_slices_concatenate_to_the_whole(codec, step):
    rfq = W.generated("pe150")
    n, ml, B, Q, lens = W.expected(rfq, row_len=160, codes=True)
    b, q, l = W.decode_rows_in_slices(codec, rfq, step, 160, codes=True)
    assert len(l) == n and np.array_equal(b, B) and np.array_equal(q, Q) and np.array_equal(l, lens)


@pytest.mark.parametrize("which", ["bases", "quals", "lens"])
def test_one_output_left_out(codec, which):
    rfq = W.generated("pe150")
    n, ml, B, Q, lens = W.expected(rfq, row_len=150)
    gn, gml, gb, gq, gl = codec.decode_rows_bytes(rfq, row_len=150, **{which: False})
    assert gn == n
    for name, got, want in (("bases", gb, B), ("quals", gq, Q), ("lens", gl, lens)):
        assert (got is None) if name == which else np.array_equal(got, want), name


def _text_rows(text, L, codes=True, qual_offset=33, pad=255):
    """rows built with torch on the device from a FASTQ text already in HBM (records of one length or several)"""
    import torch
    nl = torch.nonzero(text == 10).flatten()
    starts = torch.cat([torch.zeros(1, dtype=nl.dtype, device=nl.device), nl + 1])
    n = nl.numel() // 4
    s0, s1 = starts[1:4 * n:4], nl[1:4 * n:4]                 # sequence line [s0, s1)
    q0 = starts[3:4 * n:4]
    lens = (s1 - s0).to(torch.int32)
    lut = torch.full((256,), 255, dtype=torch.uint8, device=text.device)
    for i, b in enumerate(b"ACGTN"):
        lut[b] = i
    B = torch.full((n, L), pad, dtype=torch.uint8, device=text.device); Q = torch.full((n, L), pad, dtype=torch.uint8, device=text.device)
    ar = torch.arange(L, device=text.device)
    for a in range(0, n, 1 << 20):
        e = min(n, a + (1 << 20))
        m = ar[None, :] < lens[a:e, None]
        sb = text[(s0[a:e, None] + ar[None, :]).clamp(max=text.numel() - 1)]
        sq = text[(q0[a:e, None] + ar[None, :]).clamp(max=text.numel() - 1)]
        B[a:e] = torch.where(m, lut[sb.long()] if codes else sb, B[a:e])
        Q[a:e] = torch.where(m, ((sq.int() - qual_offset) & 255).to(torch.uint8), Q[a:e])
    return B, Q, lens


def test_large_pe150_through_decode_tensors():
    """about 2 x 256 MB of PE150 text: repaq_amd.tensors.decode_tensors against rows built on the device from rfq_decode_batch's text of the
    same image (split_pe = 0); R1 / R2 rows against the two split_pe outputs; decoding twice gives identical tensors"""
    import torch
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import decode_tensors
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    try:
        dev = torch.device("cuda:0")
        a1, a2 = O.gen_np(O.NOVA_PE150, 750_000, seed=21)
        t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
        r = c.encode(t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), PE_TWO_FILES, 1_000_000)
        rfq = torch.empty(r.rfq_len, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        import ctypes as C
        c._check(c._L.rfq_copy_d2d(c._h, C.c_void_p(rfq.data_ptr()), C.c_void_p(r.d_rfq), r.rfq_len))
        got = decode_tensors(c, rfq)
        got2 = decode_tensors(c, rfq, row_len=160)
        torch.cuda.synchronize()
        n = got["lens"].numel()
        assert n == 1_500_000 and got["bases"].shape == (n, 150)
        d = c.decode(rfq.data_ptr(), rfq.numel(), split_pe=False)
        text = torch.empty(d.n1, dtype=torch.uint8, device=dev)
        c._check(c._L.rfq_copy_d2d(c._h, C.c_void_p(text.data_ptr()), C.c_void_p(d.d_fq1), d.n1))
        B, Q, lens = _text_rows(text, 150)
        assert torch.equal(got["bases"], B) and torch.equal(got["quals"], Q) and torch.equal(got["lens"], lens)
        assert torch.equal(got2["bases"][:, :150], B) and bool((got2["bases"][:, 150:] == 255).all()) and torch.equal(got2["quals"][:, :150], Q)
        del text, B, Q
        # R1 / R2 against the split decode (its text equals the input: the suite pins that)
        B1, Q1, _ = _text_rows(t1, 150); B2, Q2, _ = _text_rows(t2, 150)
        v = got["bases"].view(-1, 2, 150); w = got["quals"].view(-1, 2, 150)
        assert torch.equal(v[:, 0], B1) and torch.equal(v[:, 1], B2) and torch.equal(w[:, 0], Q1) and torch.equal(w[:, 1], Q2)
        again = decode_tensors(c, rfq)
        assert all(torch.equal(again[k], got[k]) for k in got)
    finally:
        c.close()
