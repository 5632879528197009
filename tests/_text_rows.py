"""Shared helpers of the rfq_text_rows tests (tests/test_emu_text_rows.py on the SIMT interpreter, tests/test_gpu_text_rows.py on the MI355X).

Nothing expected comes from the code under test.  For a PLAIN text (LF only, a final newline, whole four-line records, no empty line, every quality
line as long as its sequence line) the expectation is the text's own lines, cut on the host.  For every other text - the reader's quirks: '\\r',
blank and empty lines, partial records, files of different length - it is the records of _oracle.decode_file(_oracle.encode_file(text), False): the
oracle's round trip is the reader's verdict on where records begin and end, and it is lossless on the sequence, quality and name of every record it
keeps for all such inputs of tests/golden/cases.py."""
import ctypes as C

import numpy as np

import _engine as E
import _oracle as O
import _rows as W
import _rows_enc as R
from cases import CASES


def lines_of(text: bytes):
    return text.split(b"\n")[:-1]


def plain(text: bytes) -> bool:
    if b"\r" in text or not text.endswith(b"\n"):
        return False
    ln = lines_of(text)
    if not ln or len(ln) % 4:
        return False
    return all(len(x) >= 1 for x in ln) and all(len(ln[i + 3]) == len(ln[i + 1]) for i in range(0, len(ln), 4))


def _recs(text: bytes):
    ln = lines_of(text if text.endswith(b"\n") or not text else text + b"\n")          # (the oracle's decode ends like the input did: the last line may be unterminated)
    return [(ln[i], ln[i + 1], ln[i + 3]) for i in range(0, len(ln) - len(ln) % 4, 4)]


def expect(fq1: bytes, fq2: bytes = b"", paired=O.SE, chunk_bases=1_000_000):
    """(route, [(name, sequence, quality)]) - the rows rfq_text_rows must give, in row order"""
    two = paired == O.PE_TWO_FILES
    if plain(fq1) and (not two or plain(fq2)):
        recs = _recs(fq1)
        if two:
            recs = [r for pair in zip(recs, _recs(fq2)) for r in pair]
        elif paired == O.PE_INTERLEAVED:
            recs = recs[:len(recs) - len(recs) % 2]
        return "plain", recs
    return "oracle", _recs(O.decode_file(O.encode_file(fq1, fq2 if two else b"", paired, chunk_bases), False))


def _case(name):
    c = CASES[name]
    return c["fq1"], (c.get("fq2", b"") if c["paired"] == O.PE_TWO_FILES else b""), c["paired"], c.get("k", 1000) * 1000


def _split():
    routes = {}
    for name in sorted(CASES):
        fq1, fq2, paired, cb = _case(name)
        routes[name] = expect(fq1, fq2, paired, cb)[0]
    n_plain = sum(1 for r in routes.values() if r == "plain"); n_oracle = sum(1 for r in routes.values() if r == "oracle")
    # (a parameter list that shrinks silently fails here)
    assert n_plain >= 60 and n_oracle >= 25 and n_plain + n_oracle == len(CASES) >= 91, (n_plain, n_oracle, len(CASES))
    return routes


ROUTES = _split()
CASE_NAMES = sorted(ROUTES)
CR_CASES = [n for n in CASE_NAMES if b"\r" in CASES[n]["fq1"] or b"\r" in CASES[n].get("fq2", b"")]
assert len(CR_CASES) >= 3, CR_CASES


def arrays(recs, row_len=None, extra=0, codes=False, qual_offset=33, pad_base=255, pad_qual=255):
    """(L, bases [n, L], quals [n, L], lens [n], names, first row with a base outside ACGTN or None) of expected records"""
    n = len(recs); lens = np.array([len(r[1]) for r in recs], np.int32)
    ml = int(lens.max()) if n else 0
    L = row_len if row_len is not None else ((ml // 16 + 1) * 16 if extra == "x16" else max(ml + extra, 1))
    B = np.full((n, L), pad_base, np.uint8); Q = np.full((n, L), pad_qual, np.uint8); bad = None
    for i, (_, s, q) in enumerate(recs):
        sv = np.frombuffer(s, np.uint8); qv = np.frombuffer(q[:len(s)], np.uint8)
        if codes:
            sv = W.CODE[sv]
            if bad is None and (sv == 255).any():
                bad = i
        B[i, :len(sv)] = sv
        Q[i, :len(qv)] = (qv.astype(np.int32) - qual_offset) & 0xFF
    return L, B, Q, lens, [r[0] for r in recs], bad


class DevText:
    """a text in device memory, `shift` bytes into its allocation"""
    def __init__(self, codec, text, shift=0):
        self.codec, self.n = codec, len(text)
        self.raw = codec.dev_put(b"\xEE" * shift + text)
        self.ptr = C.c_void_p(self.raw.value + shift)

    def free(self):
        self.codec.dev_free(self.raw)


def call(codec, fq1, fq2=b"", paired=O.SE, recs=None, row_len=None, extra=0, codes=False, qual_offset=33, pad_base=255, pad_qual=255, out_shift=0, in_shift=0,
         final=True, outputs="bqlno", **kw):
    """One size query and one rfq_text_rows into Guarded buffers of exactly the reported sizes, compared with `recs` (None: nothing is compared).
    Returns (result, bases, quals, lens, names) - an output not in `outputs` is not asked for (NULL) and comes back as None."""
    two = paired == O.PE_TWO_FILES
    t1 = DevText(codec, fq1, in_shift); t2 = DevText(codec, fq2, in_shift) if two else None
    gs = []
    try:
        src = dict(d_fq2=t2.ptr if two else None, n2=len(fq2) if two else 0, paired=paired, final=final, **kw)
        q = codec.text_rows(t1.ptr, len(fq1), **src)
        n, nl = int(q.n_rows), int(q.names_len)
        if recs is not None:
            L, B, Q, lens, names, bad = arrays(recs, row_len, extra, codes, qual_offset, pad_base, pad_qual)
            assert (n, q.max_len, q.n_bases, nl, q.max_name) == (len(recs), int(lens.max()) if n else 0, int(lens.sum()), sum(map(len, names)),
                                                                  max(map(len, names)) if n else 0), (n, q.max_len, q.n_bases, nl, q.max_name, len(recs))
        else:
            L = row_len if row_len is not None else max(int(q.max_len) + (extra if extra != "x16" else 16 - int(q.max_len) % 16), 1)
        gb = W.Guarded(codec, n * L, shift=out_shift) if "b" in outputs else None
        gq = W.Guarded(codec, n * L, shift=out_shift) if "q" in outputs else None
        gl = W.Guarded(codec, 4 * n) if "l" in outputs else None
        gn = W.Guarded(codec, nl, shift=out_shift) if "n" in outputs else None
        go = W.Guarded(codec, 8 * (n + 1)) if "o" in outputs else None
        gs = [g for g in (gb, gq, gl, gn, go) if g is not None]

        def p(g):
            return g.ptr if g is not None else None
        r = codec.text_rows(t1.ptr, len(fq1), row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad_base, pad_qual=pad_qual,
                            d_bases=p(gb), bases_cap=n * L if gb else 0, d_quals=p(gq), quals_cap=n * L if gq else 0, d_lens=p(gl), lens_cap=n if gl else 0,
                            d_names=p(gn), names_cap=nl if gn else 0, d_name_off=p(go), off_cap=n + 1 if go else 0, **src)
        for f in ("n_rows", "n_bases", "names_len", "max_len", "max_name", "consumed1", "consumed2", "input_ended"):
            assert getattr(r, f) == getattr(q, f), (f, getattr(r, f), getattr(q, f))
        assert all(g.guards_intact() for g in gs), "a guard around an output buffer was written"
        gB = np.frombuffer(gb.body(), np.uint8).reshape(n, L) if gb else None
        gQ = np.frombuffer(gq.body(), np.uint8).reshape(n, L) if gq else None
        gL = np.frombuffer(gl.body(), np.int32) if gl else None
        off = np.frombuffer(go.body(), np.uint64) if go else None
        blob = gn.body() if gn else None
        if off is not None:
            assert off[0] == 0 and off[n] == nl and (np.diff(off.astype(np.int64)) >= 0).all()
        gN = None
        if recs is not None:
            want_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64)
            if gL is not None: assert np.array_equal(gL, lens)
            if off is not None: assert np.array_equal(off, want_off)
            if blob is not None: assert blob == b"".join(names), "the name blob differs"
            for got, want, what in ((gB, B, "base"), (gQ, Q, "quality")):
                if got is not None and n:
                    rows = np.nonzero((got != want).any(axis=1))[0]
                    assert not len(rows), "%s rows differ: %d of %d, first %d: %r / %r" % (what, len(rows), n, rows[0], bytes(got[rows[0]][:48]), bytes(want[rows[0]][:48]))
        if blob is not None and off is not None:
            gN = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
        return r, gB, gQ, gL, gN
    finally:
        t1.free()
        if t2: t2.free()
        for g in gs: g.free()


def used_whole(r, fq1, fq2, paired, recs, cb):
    """consumed* = the stream length wherever the reader used the whole text: always for a plain text (two files: of the same record count).  For the
    others, unless the reader stopped at an empty line, what lies behind consumed is less than a record (a pair): fewer than four non-empty lines
    (interleaved: eight), with two files in at least one of them"""
    import re
    two = paired == O.PE_TWO_FILES
    if plain(fq1) and (not two or (plain(fq2) and fq1.count(b"\n") == fq2.count(b"\n"))):
        if paired != O.PE_INTERLEAVED or fq1.count(b"\n") % 8 == 0:
            assert (r.consumed1, r.consumed2) == (len(fq1), len(fq2) if two else 0), (r.consumed1, r.consumed2, len(fq1), len(fq2))
            return
    assert r.consumed1 <= len(fq1) and r.consumed2 <= len(fq2)
    if not r.input_ended:
        left = [len([x for x in re.split(b"[\r\n]", t[c:]) if x]) for t, c in ((fq1, r.consumed1), (fq2, r.consumed2))]
        assert min(left) < 4 if two else left[0] < (8 if paired == O.PE_INTERLEAVED else 4), (left, r.consumed1, r.consumed2)


# ---------------------------------------------------------------- test 1: the golden cases
def check_case(codec, name):
    from repaq_amd import RfqError
    fq1, fq2, paired, cb = _case(name)
    route, recs = expect(fq1, fq2, paired, cb)
    r = call(codec, fq1, fq2, paired, recs)[0]
    used_whole(r, fq1, fq2, paired, recs, cb)
    if name in CR_CASES:
        assert "normalise" in dict(codec.timings()), codec.timings()
    assert {"index", "text_rows:sizes", "text_rows:rows", "text_rows:names"} <= set(dict(codec.timings())) or not recs, codec.timings()
    bad = arrays(recs, codes=True)[5]
    if bad is None:
        call(codec, fq1, fq2, paired, recs, codes=True, extra="x16")
    else:
        try:
            call(codec, fq1, fq2, paired, recs, codes=True)
        except RfqError as e:
            assert e.code == -5 and "first such row: %d)" % bad in e.message, (bad, e)
        else:
            raise AssertionError("%s: code mode took a base outside ACGTN (row %d)" % (name, bad))
    return route


def good(codec):
    """what every refusal is followed by: the first golden case, on the same context"""
    check_case(codec, CASE_NAMES[0])


# ---------------------------------------------------------------- test 2: generated inputs over the row variants
GEN_LABELS = [g[0] for g in W.GENERATED]


def check_generated(codec, label):
    _, fq1, fq2, paired, cb = R.BY_LABEL[label]
    recs = expect(fq1, fq2, paired, cb)[1]
    assert 300 <= len(recs) <= 600
    for k, (codes, extra, qoff, shift) in enumerate(R.VARIANTS):
        call(codec, fq1, fq2, paired, recs, extra=extra, codes=codes, qual_offset=qoff, out_shift=shift, pad_base=(0xA7 + k) & 0xFF, pad_qual=(0x51 + k) & 0xFF)
    for in_shift in (1, 7, 15):
        for codes, extra, qoff, shift in (R.VARIANTS[0], R.VARIANTS[2]):
            call(codec, fq1, fq2, paired, recs, extra=extra, codes=codes, qual_offset=qoff, out_shift=shift, in_shift=in_shift)


# ---------------------------------------------------------------- test 3: small shapes where the writers can go wrong
def lengths_text():
    lens = list(range(1, 71)) + [127, 128, 129, 255, 256, 257]
    return E.handmade(len(lens), lambda i: "r%d" % i, lambda i: lens[i], lambda i: "+", seed=21)


def residue_text():
    """names of 2..255 bytes ('@' included): records and names start at every residue mod 16 (asserted)"""
    text = E.handmade(508, lambda i: "n" * (1 + i % 254), lambda i: (1, 15, 16, 17, 33)[(i * 3 + i // 5) % 5], lambda i: "+", seed=22)
    rec_starts, name_starts, pos, npos = set(), set(), 0, 0
    ln = lines_of(text)
    for i in range(0, len(ln), 4):
        rec_starts.add(pos % 16); name_starts.add(npos % 16); pos += sum(len(x) + 1 for x in ln[i:i + 4]); npos += len(ln[i])
    assert rec_starts == set(range(16)) and name_starts == set(range(16)) and {len(ln[i]) for i in range(0, len(ln), 4)} == set(range(2, 256))
    return text


def check_shapes(codec):
    for text in (lengths_text(), residue_text()):
        recs = expect(text)[1]
        for codes, extra, shift in ((False, 0, 0), (True, "x16", 0), (True, 1, 1)):
            call(codec, text, recs=recs, codes=codes, extra=extra, out_shift=shift)
        call(codec, text, recs=recs, in_shift=9, out_shift=3)


def check_one_record_and_final(codec):
    one = b"@only\nACGTNACGTNACGTNACG\n+x\nFFFFFFFFFFFFFFFFF#\n"
    recs = [(b"@only", b"ACGTNACGTNACGTNACG", b"FFFFFFFFFFFFFFFFF#")]
    assert expect(one)[1] == recs
    r = call(codec, one, recs=recs, codes=True)[0]
    assert r.consumed1 == len(one)
    bare = one[:-1]
    assert expect(bare) == ("oracle", recs)                                  # (the oracle agrees: an unterminated last line is a line at the end of the input)
    r = call(codec, bare, recs=recs, final=True)[0]
    assert r.consumed1 == len(bare)
    r = call(codec, bare, recs=[], final=False)[0]                           # not the end of the input: the last record is not consumed
    assert (r.n_rows, r.consumed1) == (0, 0)
    two = one + bare
    r = call(codec, two, recs=recs, final=False)[0]
    assert r.consumed1 == len(one)


def check_long_read_and_pad(codec):
    text = E.handmade(3, lambda i: "long%d" % i, lambda i: (40, 40000, 17)[i], lambda i: "+", seed=5)
    recs = expect(text)[1]
    call(codec, text, recs=recs, codes=True, extra="x16")
    call(codec, text, recs=recs, extra=1, out_shift=1)
    short = E.handmade(40, lambda i: "s%d" % i, lambda i: 1 + i % 9, lambda i: "+", seed=6)
    call(codec, short, recs=expect(short)[1], row_len=400, pad_base=7, pad_qual=9)        # rows far longer than the reads: pad fill
    call(codec, short, recs=expect(short)[1], row_len=333, pad_base=0, pad_qual=1, out_shift=1)


def check_each_output_alone(codec):
    _, fq1, fq2, paired, cb = R.BY_LABEL["se_var"]
    recs = expect(fq1, fq2, paired, cb)[1]
    for o in "bqlno":
        call(codec, fq1, fq2, paired, recs, outputs=o, codes=(o == "b"))


# ---------------------------------------------------------------- test 4: pairs
def pair_texts():
    fq1, fq2 = O.gen(O.NOVA_PE150, 240, seed=14)
    cut = b"\n".join(fq2.split(b"\n")[:4 * 200]) + b"\n"
    return fq1, fq2, cut


def check_pairs(codec):
    fq1, fq2, cut = pair_texts()
    recs = expect(fq1, cut, O.PE_TWO_FILES)[1]
    assert len(recs) == 400
    r = call(codec, fq1, cut, O.PE_TWO_FILES, recs)[0]
    assert r.consumed2 == len(cut) and r.consumed1 < len(fq1) and fq1[:r.consumed1].count(b"\n") == 800
    r = call(codec, cut, fq1, O.PE_TWO_FILES, [x for k in range(200) for x in (recs[2 * k + 1], recs[2 * k])])[0]
    assert r.consumed2 < len(fq1) and r.consumed1 == len(cut)
    l1, l2 = lines_of(fq1), lines_of(cut)
    inter = b"".join(b"\n".join(l1[4 * k:4 * k + 4]) + b"\n" + b"\n".join(l2[4 * k:4 * k + 4]) + b"\n" for k in range(200))
    r = call(codec, inter, paired=O.PE_INTERLEAVED, recs=recs, codes=True, extra="x16")[0]
    assert r.consumed1 == len(inter)
    seven = b"".join(b"\n".join(l1[4 * k:4 * k + 4]) + b"\n" for k in range(7))
    r = call(codec, seven, paired=O.PE_INTERLEAVED, recs=_recs(seven)[:6])[0]
    assert r.n_rows == 6 and seven[:r.consumed1].count(b"\n") == 24


# ---------------------------------------------------------------- test 5: streaming
def _rows_text_bytes(codec, text, final, **kw):
    r, B, Q, lens, names = call(codec, text, final=final, row_len=STREAM_L, **kw)
    return r, [(names[i], bytes(B[i][:lens[i]]), bytes(Q[i][:lens[i]])) for i in range(int(r.n_rows))]


STREAM_L = 320


def stream_text():
    _, fq1, _, _, _ = R.BY_LABEL["se_var"]
    assert fq1.count(b"\n") == 2400
    return fq1


def check_streaming(codec, step):
    text = stream_text()
    want = [(n, s, bytes((np.frombuffer(q, np.uint8) - 33).astype(np.uint8))) for n, s, q in _recs(text)]
    got, pos, end, calls = [], 0, min(step, len(text)), 0
    while True:
        final = end == len(text)
        r, rows = _rows_text_bytes(codec, text[pos:end], final)
        got += rows; calls += 1
        assert r.consumed1 <= end - pos
        if final:
            assert r.consumed1 == end - pos
            break
        pos += r.consumed1
        end = min(len(text), max(end, pos) + step)
    assert got == want and calls > 3


def check_streaming_forced_slices(codec, slice_bytes=8192):
    text = stream_text()
    want = [(n, s, bytes((np.frombuffer(q, np.uint8) - 33).astype(np.uint8))) for n, s, q in _recs(text)]
    codec.set_option("RFQ_SLICE_BYTES", str(slice_bytes))
    try:
        got, pos, short = [], 0, 0
        while pos < len(text):
            r, rows = _rows_text_bytes(codec, text[pos:], True)
            assert r.consumed1 > 0
            short += r.consumed1 < len(text) - pos
            got += rows; pos += r.consumed1
        assert got == want and short >= 3
    finally:
        codec.set_option("RFQ_SLICE_BYTES", None)


# ---------------------------------------------------------------- test 6: sizes and refusals
def check_short_caps(codec):
    from repaq_amd import RfqError
    _, fq1, fq2, paired, cb = R.BY_LABEL["pe150"]
    recs = expect(fq1, fq2, paired, cb)[1]
    L, B, Q, lens, names, _ = arrays(recs)
    n, nl = len(recs), sum(map(len, names))
    t1, t2 = DevText(codec, fq1), DevText(codec, fq2)
    g = dict(b=W.Guarded(codec, n * L), q=W.Guarded(codec, n * L), l=W.Guarded(codec, 4 * n), n=W.Guarded(codec, nl), o=W.Guarded(codec, 8 * (n + 1)))
    try:
        caps = dict(bases_cap=n * L, quals_cap=n * L, lens_cap=n, names_cap=nl, off_cap=n + 1)
        ptrs = dict(d_bases=g["b"].ptr, d_quals=g["q"].ptr, d_lens=g["l"].ptr, d_names=g["n"].ptr, d_name_off=g["o"].ptr)
        before = {k: v.body() for k, v in g.items()}
        for short in list(caps) + ["row_len"]:
            kw = dict(caps, row_len=L); kw[short] -= 1
            try:
                codec.text_rows(t1.ptr, len(fq1), t2.ptr, len(fq2), paired, **ptrs, **kw)
            except RfqError as e:
                assert e.code == -8 and "need" in e.message, (short, e)
            else:
                raise AssertionError("%s one short was accepted" % short)
            assert all(v.body() == before[k] and v.guards_intact() for k, v in g.items()), short
            good(codec)
    finally:
        t1.free(); t2.free()
        for v in g.values(): v.free()


def check_quality_lengths(codec):
    from repaq_amd import RfqError
    base = lines_of(E.handmade(9, lambda i: "q%d" % i, lambda i: 30 + i, lambda i: "+", seed=9))
    short = list(base); short[4 * 5 + 3] = short[4 * 5 + 3][:-1]
    try:
        call(codec, b"\n".join(short) + b"\n")
    except RfqError as e:
        assert e.code == -7 and "shorter than its sequence line" in e.message, e
    else:
        raise AssertionError("a quality line one short was accepted")
    good(codec)
    longer = list(base); longer[4 * 5 + 3] += b"F"
    text = b"\n".join(longer) + b"\n"
    route, recs = expect(text)                                               # the oracle decides: whatever its encode -> decode keeps
    assert route == "oracle" and len(recs) == 9
    call(codec, text, recs=recs)
    call(codec, text, recs=recs, codes=True, extra="x16")


def check_argument_refusals(codec):
    from repaq_amd import RfqError
    fq1, fq2 = O.gen(O.NOVA_PE150, 20, seed=3)
    t1, t2 = DevText(codec, fq1), DevText(codec, fq2)
    buf = codec.dev_put(b"\0" * (1 << 16))
    try:
        b = buf.value
        calls = (("paired 3", lambda: codec.text_rows(t1.ptr, len(fq1), paired=3)),
                 ("paired -1", lambda: codec.text_rows(t1.ptr, len(fq1), paired=-1)),
                 ("row_len 0", lambda: codec.text_rows(t1.ptr, len(fq1), row_len=0, d_bases=C.c_void_p(b), bases_cap=1 << 16)),
                 ("misaligned d_lens", lambda: codec.text_rows(t1.ptr, len(fq1), row_len=160, d_lens=C.c_void_p(b + 2), lens_cap=1000)),
                 ("misaligned d_name_off", lambda: codec.text_rows(t1.ptr, len(fq1), row_len=160, d_name_off=C.c_void_p(b + 4), off_cap=1000)),
                 ("d_fq2 with SE", lambda: codec.text_rows(t1.ptr, len(fq1), t2.ptr, len(fq2), paired=O.SE)),
                 ("d_fq2 with interleaved", lambda: codec.text_rows(t1.ptr, len(fq1), t2.ptr, len(fq2), paired=O.PE_INTERLEAVED)))
        for what, f in calls:
            try:
                f()
            except RfqError as e:
                assert e.code == -3, (what, e)
            else:
                raise AssertionError("%s was accepted" % what)
            good(codec)
    finally:
        t1.free(); t2.free(); codec.dev_free(buf)


def check_empty_text(codec):
    for paired in (O.SE, O.PE_TWO_FILES, O.PE_INTERLEAVED):
        r, B, Q, lens, names = call(codec, b"", b"", paired, recs=[])
        assert (r.n_rows, r.names_len, r.consumed1, r.consumed2) == (0, 0, 0, 0) and names == []


# ---------------------------------------------------------------- test 7: closing the square
def check_square(codec, label):
    _, fq1, fq2, paired, cb = R.BY_LABEL[label]
    recs = expect(fq1, fq2, paired, cb)[1]
    _, B, Q, lens, names = call(codec, fq1, fq2, paired, recs, extra="x16", qual_offset=33)
    got = codec.rows_to_text_bytes(B, Q, lens, names, paired=paired)
    assert got == ((fq1, fq2) if paired == O.PE_TWO_FILES else fq1)
    codec.clearHeader()
    img = codec.encode_rows_bytes(B, Q, lens, names, paired=paired, chunk_bases=cb, **E.nolb_args(fq1, fq2, paired))
    assert img == O.encode_file(fq1, fq2, paired, cb), (label, len(img))


# ---------------------------------------------------------------- test 8: junk that is still input
def junk_texts():
    import random
    rng = random.Random(77)
    rec = b"@j\nACGT\n+\nFFFF\n"
    return [("no_newline", b"ACGT" * 1500), ("one_line_200k", b"@" + b"A" * 200000 + b"\n"),
            ("nul_and_ff", rec + b"@n\0me\nAC\0\xffGT\n+\nFF\0\xffFF\n" + rec), ("random_64k", bytes(rng.getrandbits(8) for _ in range(65536))),
            ("only_newlines", b"\n" * 3000), ("cr_soup", (b"\r\n\r" + rec) * 50)]


def run_junk(codec):
    """every junk text, final and not, SE and interleaved, returns rows or an RFQ_E_* code; the next good call on the context is right"""
    from repaq_amd import RfqError
    summary = {"calls": 0, "rows": 0, "errors": {}}
    for label, text in junk_texts():
        for paired in (O.SE, O.PE_INTERLEAVED, O.PE_TWO_FILES):
            for final in (True, False):
                for codes in (False, True):
                    try:
                        r = call(codec, text, text[::-1] if paired == O.PE_TWO_FILES else b"", paired, None, final=final, codes=codes, extra="x16")[0]
                        summary["rows"] += int(r.n_rows)
                    except RfqError as e:
                        assert e.code in (-5, -7), (label, e)                       # (RFQ_E_DATA, RFQ_E_UNPINNED: the arguments are valid and the buffers are of the reported sizes)
                        summary["errors"][str(e.code)] = summary["errors"].get(str(e.code), 0) + 1
                    summary["calls"] += 1
        good(codec)
    return summary


def write_fixtures(workdir):
    """the texts of the stand-alone sanitizer program (tools/text_rows_asan.sh): two good inputs and the junk"""
    import os
    out = []
    texts = [("se_var", R.BY_LABEL["se_var"][1]), ("lengths", lengths_text()), ("residues", residue_text()),
             ("crlf", R.BY_LABEL["se150_manyN"][1][:40000].replace(b"\n", b"\r\n"))] + junk_texts()
    for label, text in texts:
        p = os.path.join(workdir, label + ".fq")
        with open(p, "wb") as f:
            f.write(text)
        out.append(p)
    return out
