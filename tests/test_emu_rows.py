"""CPU: rfq_decode_rows - the reads of an image as fixed-stride base / quality rows - under the SIMT interpreter, against rows built from the
plain-C oracle's text (tests/_rows.py).  The GPU twins are tests/test_gpu_rows.py and tests/test_gpu_rows_hostile.py."""
import numpy as np
import pytest

import _engine as E
import _oracle as O
import _rows as W
from cases import CASES
from repaq_amd import RfqError


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.build_emu())
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
    rfq = W.generated(label)
    assert W.check(codec, rfq, codes=True) > 100


@pytest.mark.parametrize("qual_offset,extra,codes", [(0, 0, False), (33, 1, True), (64, 1, False), (33, "x16", True), (0, "x16", False)])
@pytest.mark.parametrize("label", ["pe150", "se_var"])
def test_row_len_and_offset_variants(codec, label, qual_offset, extra, codes):
    """row_len = max_len, max_len + 1 (byte-granular stores) and a multiple of 16 (whole 16-byte groups), raw and offset qualities, other pads"""
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
            assert q.n_bases == sum(len(s) for s in W.records(O.decode_file(rfq, False))[0])
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
            assert "need" in ei.value.message, ei.value.message
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


def test_bad_arguments(codec):
    rfq = W.generated("se_var"); d = codec.dev_put(rfq); o = codec.dev_put(b"\0" * 64)
    try:
        with pytest.raises(RfqError) as ei:
            codec.decode_rows(d, len(rfq), row_len=0, d_bases=o, bases_cap=64)
        assert ei.value.code == -3
        with pytest.raises(RfqError) as ei:
            codec.decode_rows(d, len(rfq), row_len=160, d_lens=o.value + 2, lens_cap=4)
        assert ei.value.code == -3
    finally:
        codec.dev_free(d); codec.dev_free(o)


@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_ranges_forced_by_slice_bases(codec, walk):
    rfq = W.generated("pe150")
    codec.set_option("RFQ_SLICE_BASES", str(45000))                    # two or three chunks of 20 k bases per range
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    W.check(codec, rfq, row_len=160, codes=True)
    names = dict(codec.timings())
    assert {"walk", "read_table", "streams", "rows"} <= set(names), names


@pytest.mark.parametrize("index", [False, True], ids=["walked", "indexed"])
def test_exact_walk(codec, index):
    rfq = W.generated("bgi_q40")
    codec.set_option("RFQ_WALK", "exact")
    W.check(codec, rfq, codes=False, chunk_off=O.chunk_table(rfq) if index else None)


def test_materialise_switch_changes_nothing(codec):
    rfq = W.generated("se150_manyN")
    codec.set_option("RFQ_MATERIALISE", "1")
    W.check(codec, rfq, codes=True)


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


def test_rows_equal_the_text_decode_of_the_same_context(codec):
    """R1 / R2 rows against the two split_pe outputs of rfq_decode_batch (row 2k = R1 of pair k, row 2k + 1 its R2)"""
    rfq = W.generated("bgi_q40")
    t1, t2 = codec.decode_bytes(rfq, split_pe=True)
    _, _, B1, Q1, _ = W.expected(rfq, row_len=112, text=t1)
    _, _, B2, Q2, _ = W.expected(rfq, row_len=112, text=t2)
    n, ml, gb, gq, gl = codec.decode_rows_bytes(rfq, row_len=112)
    assert n == 2 * len(B1)
    assert np.array_equal(gb.reshape(-1, 2, 112)[:, 0], B1) and np.array_equal(gb.reshape(-1, 2, 112)[:, 1], B2)
    assert np.array_equal(gq.reshape(-1, 2, 112)[:, 0], Q1) and np.array_equal(gq.reshape(-1, 2, 112)[:, 1], Q2)


def test_empty_image(codec):
    q = codec.decode_rows(codec.dev_put(b"x"), 0)
    assert (q.n_rows, q.max_len, q.n_chunks) == (0, 0, 0)


HOSTILE_COUNTS = dict(flip=10, header=5, fixed=8, lengths=5, quality=5, index=12)


def test_hostile_images_tame_subset(codec):
    s = W.run_hostile(codec, counts=HOSTILE_COUNTS, good_every=8, tame=True, time_bound_s=30.0)
    assert s["mutants"] >= 150 and s["good_checks"] >= 20 and s["errors"].get("FORMAT", 0) > 20 and s["decoded"] > 20, s
