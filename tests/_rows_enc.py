"""Shared helpers of the rfq_rows_to_text / rfq_encode_rows tests (tests/test_emu_rows_encode.py on the SIMT interpreter, tests/test_gpu_rows_encode.py
on the MI355X).

Nothing expected comes from the code under test: the expected text is the input's own FASTQ text, the expected image is _oracle.encode_file of it
(which the golden tests pin to the reference), and the rows and names the calls are fed are cut from the text on the host with numpy."""
import ctypes as C

import numpy as np

import _engine as E
import _oracle as O
import _rows as W
from cases import CASES


def lines_of(text: bytes):
    return text.split(b"\n")[:-1]


def plain(text: bytes) -> bool:
    """a text rows can stand for: LF only, a final newline, whole four-line records, strand line "+", non-empty reads whose quality line has the
    read's length (a row has one length), names of 1..255 bytes"""
    if b"\r" in text or not text.endswith(b"\n"):
        return False
    ln = lines_of(text)
    if not ln or len(ln) % 4:
        return False
    return all(1 <= len(ln[i]) <= 255 and len(ln[i + 1]) >= 1 and ln[i + 2] == b"+" and len(ln[i + 3]) == len(ln[i + 1]) for i in range(0, len(ln), 4))


def _inputs():
    out = []
    for name in sorted(CASES):
        c = CASES[name]; fq1, fq2, paired, cb = c["fq1"], c.get("fq2", b""), c["paired"], c.get("k", 1000) * 1000
        two = paired == O.PE_TWO_FILES
        if not plain(fq1) or (two and (not plain(fq2) or fq1.count(b"\n") != fq2.count(b"\n"))):
            continue
        try:
            O.encode_file(fq1, fq2, paired, cb)
        except O.OracleError:
            continue
        out.append((name, fq1, fq2 if two else b"", paired, cb))
    n_cases = len(out)
    for label, prof, reads, seed, cb, paired, kw in W.GENERATED:
        fq1, fq2 = O.gen(prof, reads, seed=seed, **kw)
        out.append((label, fq1, fq2 if paired == O.PE_TWO_FILES else b"", paired, cb))
    return out, n_cases


INPUTS, N_PLAIN_CASES = _inputs()
BY_LABEL = {i[0]: i for i in INPUTS}
LABELS = [i[0] for i in INPUTS]


def rows_of(fq1: bytes, fq2: bytes = b"", paired=O.SE, row_len=None, extra=0, codes=False, qual_offset=33, pad=255):
    """(bases [n, L], quals [n, L], lens [n], names) of a plain text - for PE_TWO_FILES rows 2k / 2k + 1 are record k of fq1 / fq2.  row_len None:
    the longest read + extra, or ("x16") the next multiple of 16 above it.  codes: None when a base is not one of ACGTN."""
    l1 = lines_of(fq1)
    recs = [(l1[i], l1[i + 1], l1[i + 3]) for i in range(0, len(l1), 4)]
    if paired == O.PE_TWO_FILES:
        l2 = lines_of(fq2)
        r2 = [(l2[i], l2[i + 1], l2[i + 3]) for i in range(0, len(l2), 4)]
        recs = [r for pair in zip(recs, r2) for r in pair]
    n = len(recs); lens = np.array([len(r[1]) for r in recs], np.int32)
    ml = int(lens.max()) if n else 1
    L = row_len if row_len is not None else ((ml // 16 + 1) * 16 if extra == "x16" else ml + extra)
    B = np.full((n, L), pad, np.uint8); Q = np.full((n, L), pad, np.uint8)
    for i, (_, s, q) in enumerate(recs):
        sv = np.frombuffer(s, np.uint8); qv = np.frombuffer(q, np.uint8)
        if codes:
            sv = W.CODE[sv]
            if (sv == 255).any():
                return None
        B[i, :len(sv)] = sv
        Q[i, :len(qv)] = (qv.astype(np.int32) - qual_offset) & 0xFF
    return B, Q, lens, [r[0] for r in recs]


def text_of(codec, dev, paired, want1: bytes, want2: bytes = b"", **kw):
    """rfq_rows_to_text into guarded caller buffers of exactly the texts' sizes: the size query, the texts, the guards"""
    two = paired == O.PE_TWO_FILES
    q = codec.rows_to_text(*dev.args(), paired=paired, size_only=True, **kw)
    assert (q.n1, q.n2) == (len(want1), len(want2) if two else 0), ((q.n1, q.n2), (len(want1), len(want2)))
    assert q.n_reads == dev.args()[0]
    g1 = W.Guarded(codec, len(want1)); g2 = W.Guarded(codec, len(want2)) if two else None
    try:
        assert g1.ptr.value % 16 == 0
        r = codec.rows_to_text(*dev.args(), paired=paired, d_out1=g1.ptr, cap1=len(want1), d_out2=g2.ptr if two else None, cap2=len(want2) if two else 0, **kw)
        assert (r.n1, r.n2) == (q.n1, q.n2) and r.n_bases == q.n_bases
        got1 = g1.body(); got2 = g2.body() if two else b""
        assert got1 == want1, "text 1 differs at byte %d of %d" % (next((i for i, (a, b) in enumerate(zip(got1, want1)) if a != b), -1), len(want1))
        assert got2 == want2, "text 2 differs at byte %d of %d" % (next((i for i, (a, b) in enumerate(zip(got2, want2)) if a != b), -1), len(want2))
        assert g1.guards_intact() and (g2 is None or g2.guards_intact())
        return r
    finally:
        g1.free()
        if g2:
            g2.free()


# (base mode, row_len rule, quality offset, misalignment): every value of every axis at least once, the 16-byte group loads (x16, aligned) in both modes
VARIANTS = [(False, 0, 33, 0), (True, 1, 0, 1), (True, "x16", 64, 0), (False, "x16", 0, 0), (False, 1, 64, 1), (True, 0, 33, 1), (False, "x16", 33, 1)]


def check_text_variants(codec, label):
    """test 1: rfq_rows_to_text == the input's own text(s), over VARIANTS; returns the number of variants that ran (codes need ACGTN)"""
    _, fq1, fq2, paired, _ = BY_LABEL[label]
    ran = 0
    for codes, extra, qoff, shift in VARIANTS:
        rows = rows_of(fq1, fq2, paired, extra=extra, codes=codes, qual_offset=qoff, pad=(0xA7 + ran) & 0xFF)
        if rows is None:
            continue
        dev = W.DevRows(codec, *rows, shift=shift)
        try:
            text_of(codec, dev, paired, fq1, fq2, codes=codes, qual_offset=qoff)
        finally:
            dev.free()
        ran += 1
    return ran


# inputs whose image does not hold the text's reads (judged by the oracle's decode alone): a length over 65535 does not fit the format's length field, and
# a base that is not N under the N quality comes back as N
LOSSY = {"se_len_over_65535", "se_nqual_on_non_n_before_first_n"}


def check_image(codec, label):
    """test 2: rfq_encode_rows == the oracle's image of the text.  Where the format keeps the reads whole (the oracle decodes the image back to the
    text's bases and qualities; it does not for a read over 65535 bases, an N quality on a base that is not N, an odd interleaved record count),
    the rows rfq_decode_rows gives for that image + the text's names must re-encode to the same image.  Returns whether that second leg ran."""
    _, fq1, fq2, paired, cb = BY_LABEL[label]
    want = O.encode_file(fq1, fq2, paired, cb)
    kw = E.nolb_args(fq1, fq2, paired)
    B, Q, lens, names = rows_of(fq1, fq2, paired)
    codec.clearHeader()
    got = codec.encode_rows_bytes(B, Q, lens, names, paired=paired, chunk_bases=cb, **kw)
    assert got == want, (label, len(got), len(want))
    on, _, oB, oQ, ol = W.expected(want)                                       # (the oracle's decode of the image, as rows)
    if on != len(names) or not (np.array_equal(ol, lens) and np.array_equal(oB, B) and np.array_equal(oQ, Q)):
        return False
    n, ml, gb, gq, gl = codec.decode_rows_bytes(want)
    assert n == len(names) and np.array_equal(gl, lens)
    codec.clearHeader()
    again = codec.encode_rows_bytes(gb, gq, gl, names, paired=paired, chunk_bases=cb, **kw)
    assert again == want, (label, "rows of rfq_decode_rows", len(again), len(want))
    return True


# ---------------------------------------------------------------- test 3: small shapes where the writer can go wrong
def residue_set():
    """600 SE reads of 1, 15, 16, 17, 31, 32, 33 bases under names of 2..40 bytes ('@' included): several workgroups of the writer share the text,
    and the records start at every residue mod 16 (asserted)"""
    lens = (1, 15, 16, 17, 31, 32, 33)
    text = E.handmade(600, lambda i: "n" * (1 + (i * 7) % 39), lambda i: lens[(i * 3 + i // 7) % 7], lambda i: "+", seed=12)
    starts, pos = set(), 0
    ln = lines_of(text)
    for i in range(0, len(ln), 4):
        starts.add(pos % 16); pos += sum(len(x) + 1 for x in ln[i:i + 4])
    assert starts == set(range(16)) and len(text) > 2 * 16384 and {len(ln[i]) for i in range(0, len(ln), 4)} == set(range(2, 41))
    return text


def long_read():
    return E.handmade(3, lambda i: "long%d" % i, lambda i: (40, 70000, 17)[i], lambda i: "+", seed=5)


def check_shape(codec, text, chunk_bases=20000):
    """a handmade SE text: rows -> the text (both base modes, both load paths) and -> the oracle's image"""
    for codes, extra, shift in ((False, 0, 0), (True, "x16", 0), (True, 1, 1)):
        dev = W.DevRows(codec, *rows_of(text, codes=codes, extra=extra), shift=shift)
        try:
            text_of(codec, dev, O.SE, text, codes=codes)
        finally:
            dev.free()
    codec.clearHeader()
    B, Q, lens, names = rows_of(text, codes=True)
    assert codec.encode_rows_bytes(B, Q, lens, names, chunk_bases=chunk_bases, codes=True, **E.nolb_args(text, b"", O.SE)) == O.encode_file(text, b"", O.SE, chunk_bases)


def check_no_rows(codec):
    Z = np.zeros((0, 8), np.uint8)
    for paired in (O.SE, O.PE_TWO_FILES, O.PE_INTERLEAVED):
        got = codec.rows_to_text_bytes(Z, Z, np.zeros(0, np.int32), [], paired=paired)
        assert got == ((b"", b"") if paired == O.PE_TWO_FILES else b"")
        codec.clearHeader()
        img = codec.encode_rows_bytes(Z, Z, np.zeros(0, np.int32), [], paired=paired)
        codec.clearHeader()
        assert img == codec.encode_bytes(b"", b"", paired)


# ---------------------------------------------------------------- test 4: the size query and caps one byte short
def check_sizes_and_short_caps(codec, label):
    from repaq_amd import RfqError
    _, fq1, fq2, paired, _ = BY_LABEL[label]
    two = paired == O.PE_TWO_FILES
    dev = W.DevRows(codec, *rows_of(fq1, fq2, paired))
    g1 = W.Guarded(codec, len(fq1)); g2 = W.Guarded(codec, max(len(fq2), 1))
    try:
        q = codec.rows_to_text(*dev.args(), paired=paired, size_only=True)
        assert (q.n1, q.n2) == (len(fq1), len(fq2)) and q.d_fq1 is None
        assert q.n_bases == sum(len(x) for t in (fq1, fq2) for x in lines_of(t)[1::4])
        before = (g1.body(), g2.body())
        shorts = [(len(fq1) - 1, len(fq2))] + ([(len(fq1), len(fq2) - 1)] if two else [])
        for cap1, cap2 in shorts:
            with pytest_raises(RfqError) as ei:
                codec.rows_to_text(*dev.args(), paired=paired, d_out1=g1.ptr, cap1=cap1, d_out2=g2.ptr if two else None, cap2=cap2 if two else 0)
            assert ei.value.code == -8 and "need %d" % len(fq1) in ei.value.message, ei.value
            assert (g1.body(), g2.body()) == before and g1.guards_intact() and g2.guards_intact()
        text_of(codec, dev, paired, fq1, fq2)
    finally:
        dev.free(); g1.free(); g2.free()


def pytest_raises(exc):
    import pytest
    return pytest.raises(exc)


# ---------------------------------------------------------------- test 5: every refusal, and a good call on the same context right behind it
def _base_rows(codes):
    fq1, _ = O.gen(O.NOVA_SE150, 40, seed=8)
    return fq1, rows_of(fq1, codes=codes, extra=2)


def _set(arr, i, j, v):
    arr = arr.copy(); arr[i, j] = v; return arr


def _refusals():
    """(label, expected code, codes, mutation of (B, Q, lens, names) -> (B, Q, lens, names, name_off or None, names_len delta))"""
    out = []

    def add(label, code, codes, f):
        out.append((label, code, codes, f))
    add("negative_length", -3, False, lambda B, Q, l, n: (B, Q, np.where(np.arange(len(l)) == 7, -1, l), n, None, 0))
    add("length_over_row_len", -3, False, lambda B, Q, l, n: (B, Q, np.where(np.arange(len(l)) == 39, B.shape[1] + 1, l), n, None, 0))
    add("name_offsets_decrease", -3, False, lambda B, Q, l, n: (B, Q, l, n, "swap", 0))
    add("last_offset_past_names_len", -3, False, lambda B, Q, l, n: (B, Q, l, n, None, -1))
    add("length_zero", -5, False, lambda B, Q, l, n: (B, Q, np.where(np.arange(len(l)) == 0, 0, l), n, None, 0))
    add("name_of_no_bytes", -5, False, lambda B, Q, l, n: (B, Q, l, n[:5] + [b""] + n[6:], None, 0))
    for where, j in (("line_start", 0), ("mid_line", 70), ("line_end", 149)):
        add("code_5_" + where, -5, True, lambda B, Q, l, n, j=j: (_set(B, 3, j, 5), Q, l, n, None, 0))
        add("code_255_" + where, -5, True, lambda B, Q, l, n, j=j: (_set(B, 38, j, 255), Q, l, n, None, 0))
        add("base_space_" + where, -5, False, lambda B, Q, l, n, j=j: (_set(B, 3, j, 0x20), Q, l, n, None, 0))
        add("base_del_" + where, -5, False, lambda B, Q, l, n, j=j: (_set(B, 3, j, 0x7F), Q, l, n, None, 0))
        add("base_newline_" + where, -5, False, lambda B, Q, l, n, j=j: (_set(B, 20, j, 10), Q, l, n, None, 0))
        add("qual_below_" + where, -5, False, lambda B, Q, l, n, j=j: (B, _set(Q, 9, j, (0x20 - 33) & 0xFF), l, n, None, 0))
        add("qual_above_" + where, -5, False, lambda B, Q, l, n, j=j: (B, _set(Q, 9, j, 0x7F - 33), l, n, None, 0))
    for ch, nm in ((b"\n", "newline"), (b"\r", "cr")):
        add("name_%s_mid" % nm, -5, False, lambda B, Q, l, n, ch=ch: (B, Q, l, n[:11] + [n[11][:20] + ch + n[11][21:]] + n[12:], None, 0))
        add("name_%s_end" % nm, -5, False, lambda B, Q, l, n, ch=ch: (B, Q, l, n[:11] + [n[11][:-1] + ch] + n[12:], None, 0))
    return out


REFUSALS = _refusals()
REFUSAL_IDS = [r[0] for r in REFUSALS]


def check_refusal(codec, label, through_encoder):
    """one refusal returns its code from rfq_rows_to_text (or rfq_encode_rows), and the good rows give the right text right after on the same context"""
    from repaq_amd import RfqError
    _, code, codes, mutate = REFUSALS[REFUSAL_IDS.index(label)]
    text, (B, Q, lens, names) = _base_rows(codes)
    assert all(len(x) > 30 for x in names) and (lens == 150).all()
    mB, mQ, ml, mn, off, dlen = mutate(B, Q, lens, list(names))
    name_off = None
    if off == "swap":
        name_off = np.concatenate([[0], np.cumsum([len(x) for x in mn])]).astype(np.uint64); name_off[[4, 5]] = name_off[[5, 4]]
    bad = W.DevRows(codec, mB, mQ, ml, mn, name_off=name_off); good = W.DevRows(codec, B, Q, lens, names)
    try:
        args = list(bad.args()); args[6] += dlen
        with pytest_raises(RfqError) as ei:
            if through_encoder:
                codec.clearHeader(); codec.encode_rows(*args, codes=codes)
            else:
                codec.rows_to_text(*args, codes=codes)
        assert ei.value.code == code, (label, ei.value)
        if through_encoder:
            assert not {"index", "gather", "assemble"} & set(dict(codec.timings())), codec.timings()          # (the encoder was not run)
        text_of(codec, good, O.SE, text, codes=codes)
    finally:
        bad.free(); good.free()


def check_argument_refusals(codec):
    from repaq_amd import RfqError
    text, (B, Q, lens, names) = _base_rows(False)
    odd = W.DevRows(codec, B[:39], Q[:39], lens[:39], names[:39]); good = W.DevRows(codec, B, Q, lens, names)
    try:
        for what, call in (("odd rows, two files", lambda: codec.rows_to_text(*odd.args(), paired=O.PE_TWO_FILES)),
                           ("odd rows, two files, encoder", lambda: codec.encode_rows(*odd.args(), paired=O.PE_TWO_FILES)),
                           ("neither final nor flush_all", lambda: codec.encode_rows(*good.args(), final=False, flush_all=False)),
                           ("a text pointer in enc", lambda: codec.encode_rows(*good.args(), d_fq1=good.args()[2])),
                           ("row_len 0", lambda: codec.rows_to_text(good.args()[0], 0, *good.args()[2:])),
                           ("misaligned output", lambda: codec.rows_to_text(*good.args(), d_out1=C.c_void_p(good.bases.value + 8), cap1=1 << 20))):
            codec.clearHeader()
            with pytest_raises(RfqError) as ei:
                call()
            assert ei.value.code == -3, (what, ei.value)
            text_of(codec, good, O.SE, text)
    finally:
        odd.free(); good.free()


# ---------------------------------------------------------------- test 6: two row batches make one file
def check_two_batches(codec, label="se_var", cut=250):
    _, fq1, fq2, paired, cb = BY_LABEL[label]
    two = paired == O.PE_TWO_FILES

    def split(t):
        ln = t.split(b"\n"); a = b"\n".join(ln[:4 * cut]) + b"\n"
        return a, t[len(a):]
    (a1, b1), (a2, b2) = split(fq1), (split(fq2) if two else (b"", b""))
    codec.clearHeader()
    want = codec.encode_bytes(a1, a2, paired, cb, final=False, flush_all=True, emit_header=True) + \
        codec.encode_bytes(b1, b2, paired, cb, final=True, emit_header=False, file_off1=len(a1), file_off2=len(a2))
    assert O.decode_file(want, two) == ((fq1, fq2) if two else fq1)
    codec.clearHeader()
    got = codec.encode_rows_bytes(*rows_of(a1, a2, paired), paired=paired, chunk_bases=cb, final=False, flush_all=True, emit_header=True) + \
        codec.encode_rows_bytes(*rows_of(b1, b2, paired, codes=True), paired=paired, chunk_bases=cb, codes=True, final=True, emit_header=False,
                                file_off1=len(a1), file_off2=len(a2))
    assert got == want, (len(got), len(want))


def check_stage_names(codec):
    """rows_sizes and rows_text lead rfq_last_timings, the encoder's own stages follow"""
    text, (B, Q, lens, names) = _base_rows(False)
    codec.clearHeader()
    codec.encode_rows_bytes(B, Q, lens, names)
    t = [n for n, _ in codec.timings()]
    assert t[:2] == ["rows_sizes", "rows_text"] and "index" in t[2:] and "assemble" in t[2:], t
    codec.rows_to_text_bytes(B, Q, lens, names)
    assert [n for n, _ in codec.timings()] == ["rows_sizes", "rows_text"]
