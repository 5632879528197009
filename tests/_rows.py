"""Shared helpers of the rfq_decode_rows tests (tests/test_emu_rows.py on the SIMT interpreter, tests/test_gpu_rows*.py on the MI355X).

The expected rows never come from the kernel: the plain-C oracle decodes the image to text (_oracle.decode_file(rfq, False): Repaq::decompress
order), the text is cut into four-line records on the host and the arrays are built with numpy."""
import ctypes as C
import time

import numpy as np

import _hostile as H
import _oracle as O

CODE = np.full(256, 255, np.uint8)
for _i, _b in enumerate(b"ACGTN"):
    CODE[_b] = _i

# MULTI-style generated inputs: (label, profile, reads, seed, chunk bases, paired, generator kwargs)
GENERATED = [
    ("se150_manyN", O.NOVA_SE150, 600, 2, 20000, O.SE, dict(nppm=5000)),
    ("se_var", O.SE_VAR, 600, 3, 15000, O.SE, {}),
    ("pe150", O.NOVA_PE150, 300, 4, 20000, O.PE_TWO_FILES, {}),
    ("bgi_q40", O.BGI_PE100, 300, 5, 10000, O.PE_TWO_FILES, dict(n_quals=40)),
]


def generated(label):
    for g in GENERATED:
        if g[0] == label:
            _, prof, reads, seed, cb, paired, kw = g
            fq1, fq2 = O.gen(prof, reads, seed=seed, **kw)
            return O.encode_file(fq1, fq2, paired, cb)
    raise KeyError(label)


def records(text: bytes):
    """(sequence lines, quality lines) of a FASTQ text"""
    lines = text.split(b"\n")
    n = len(lines) // 4
    return [lines[4 * i + 1] for i in range(n)], [lines[4 * i + 3] for i in range(n)]


def expected(rfq: bytes, row_len=None, codes=False, qual_offset=33, pad_base=255, pad_qual=255, text=None):
    """(n_rows, max_len, bases, quals, lens) as rfq_decode_rows must write them, from the oracle's text"""
    seqs, quals = records(O.decode_file(rfq, False) if text is None else text)
    n = len(seqs); lens = np.array([len(s) for s in seqs], np.int32)
    ml = int(lens.max()) if n else 0
    L = max(ml, 1) if row_len is None else row_len
    B = np.full((n, L), pad_base, np.uint8); Q = np.full((n, L), pad_qual, np.uint8)
    for i, (s, q) in enumerate(zip(seqs, quals)):
        sv = np.frombuffer(s, np.uint8); qv = np.frombuffer(q, np.uint8)
        B[i, :len(sv)] = CODE[sv] if codes else sv
        Q[i, :len(qv)] = (qv.astype(np.int32) - qual_offset) & 0xFF
    return n, ml, B, Q, lens


def check(codec, rfq: bytes, row_len=None, codes=False, qual_offset=33, pad_base=255, pad_qual=255, **kw):
    """rfq_decode_rows on the image == the oracle's rows; returns the number of rows"""
    n, ml, B, Q, lens = expected(rfq, row_len, codes, qual_offset, pad_base, pad_qual)
    gn, gml, gb, gq, gl = codec.decode_rows_bytes(rfq, row_len=row_len, codes=codes, qual_offset=qual_offset, pad_base=pad_base, pad_qual=pad_qual, **kw)
    assert (gn, gml) == (n, ml), ((gn, gml), (n, ml))
    assert np.array_equal(gl, lens)
    if n:
        bad = np.nonzero((gb != B).any(axis=1) | (gq != Q).any(axis=1))[0]
        assert not len(bad), "rows differ from the oracle: %d of %d, first %d: %r / %r" % (len(bad), n, bad[0], bytes(gb[bad[0]][:48]), bytes(B[bad[0]][:48]))
    return n


class Guarded:
    """a device buffer of `n` bytes with `guard` bytes of 0xA5 on either side (and `shift` bytes more in front: a misaligned start)"""
    def __init__(self, codec, n, guard=64, shift=0):
        self.codec, self.n, self.front, self.back = codec, n, guard + shift, guard
        self.raw = codec.dev_put(b"\xA5" * (n + 2 * guard + shift))
        self.ptr = C.c_void_p(self.raw.value + self.front)

    def body(self):
        return self.codec.dev_get(self.ptr, self.n) if self.n else b""

    def guards_intact(self):
        front = self.codec.dev_get(self.raw, self.front); back = self.codec.dev_get(C.c_void_p(self.raw.value + self.front + self.n), self.back)
        return set(front) <= {0xA5} and set(back) <= {0xA5}

    def free(self):
        self.codec.dev_free(self.raw)


def walk_counts(row_len, iters):
    """the unit counts at which the walk of a deciding call's common-path kernel has a seam (enc/rows_lanes.h, UnitGroup): a group of LPR lanes takes a unit, G =
    64 / LPR units a wave, R = 256 / LPR a workgroup's step, R * iters a workgroup - one less, exactly and one more of each, and a third workgroup begun.  LPR is
    16 up to row_len 256 and 64 up to 1024; beyond that a wave takes a unit and a few counts do.  (G - 1 is 0 at LPR 64: the call of no rows.)"""
    if row_len > 1024:
        return [1, 2, 5]
    lpr = 16 if row_len <= 256 else 64
    R, G = 256 // lpr, 64 // lpr
    return sorted({1, G - 1, G, G + 1, R - 1, R, R + 1, R * iters - 1, R * iters, R * iters + 1, 2 * R * iters + G + 1})


# (row_len, the call's `general` option, all the walk's counts): 256 the last row length of the <16> kernel, 272 the first of <64>, 1024 its last, 1040 the first of
# the wave-per-unit kernel
WALK_CASES = [(256, None, True), (272, None, True), (272, "general", True), (1024, None, False), (1040, None, False)]
WALK_IDS = ["%d%s" % (L, "_" + p if p else "") for L, p, _ in WALK_CASES]


def walk_case(label, iters):
    """(row_len, option, unit counts) of a WALK_IDS label"""
    L, path, every = WALK_CASES[WALK_IDS.index(label)]
    return L, path, (walk_counts(L, iters) if every else [1, 2, 5])


class DevRows:
    """Rows in device memory as the rows calls take them: base rows, optionally quality rows (Q None: NULL), lengths, optionally names (None: rows without names;
    name_off: other offsets than the names' own).  shift: bytes by which the row buffers and the name blob are moved off their 256-byte aligned start.  Every
    buffer ends where its allocation's payload ends, so a read behind the last row shows under the sanitizer build.  extra: further inputs of the call, name =
    (array or None, dtype) - each becomes the attribute `name`, a device pointer or None for a NULL argument (_select.dev_sel: keep, start, length; _merge.dev_merge:
    insert).  put(): one more buffer, freed with the rest."""
    def __init__(self, codec, B, Q, lens, names=None, shift=0, name_off=None, **extra):
        self.codec = codec; self.n, self.L = B.shape; self.raw = []
        self.bases = self.put(np.ascontiguousarray(B, np.uint8).tobytes(), shift)
        self.quals = self.put(np.ascontiguousarray(Q, np.uint8).tobytes(), shift) if Q is not None else None
        self.lens = self.put(np.ascontiguousarray(lens, np.int32).tobytes())
        self.names = self.name_off = None; self.names_len = 0
        if names is not None:
            off = np.zeros(self.n + 1, np.uint64)
            if self.n:
                off[1:] = np.cumsum([len(x) for x in names])
            if name_off is not None:
                off = np.asarray(name_off, np.uint64)
            blob = b"".join(names); self.names_len = len(blob)
            self.names = self.put(blob, shift); self.name_off = self.put(off.tobytes())
        for name, (v, dtype) in extra.items():
            setattr(self, name, self.put(np.ascontiguousarray(v, dtype).tobytes()) if v is not None else None)

    def put(self, data, shift=0):
        r = self.codec.dev_put(b"\xEE" * shift + data); self.raw.append(r)
        return C.c_void_p(r.value + shift)

    def args(self):
        """rfq_rows_in: what rfq_select_rows, rfq_merge_rows, rfq_rows_to_text and rfq_encode_rows take"""
        return (self.n, self.L, self.bases, self.quals, self.lens, self.names, self.names_len, self.name_off)

    def judge_args(self):
        return (self.n, self.L, self.bases, self.quals, self.lens)

    def adapter_args(self):
        return (self.n, self.L, self.bases, self.lens)

    def free(self):
        for r in self.raw:
            self.codec.dev_free(r)


def padded(rows, L, pad):
    out = np.full((len(rows), L), pad, np.uint8)
    for j, r in enumerate(rows):
        out[j, :len(r)] = np.frombuffer(r, np.uint8)
    return out


def compact_into_guarded(codec, call, e, L, pad_base, pad_qual, outputs="bqlno", out_shift=0, what="", rows_differ=None):
    """The second call of a compacting call (rfq_select_rows, rfq_merge_rows) after its size query: call(**outputs and caps) writes into Guarded buffers of exactly
    the sizes `e` (the caller's expected dict: idx, lens, bases, quals, names, names_len) gives at stride L; the guards, lens, name offsets, name blob and padded
    rows are compared with `e`.  what: prefix of the failure messages; rows_differ(kind, got, want, bad rows) words the caller's own for rows.  Returns
    (result, bases, quals, lens, raw) - an output not in `outputs` is not asked for and comes back as None; raw: the bytes of every output body."""
    n, nl = len(e["idx"]), e["names_len"]
    size = dict(b=n * L, q=n * L, l=4 * n, n=nl, o=8 * (n + 1))
    g = {o: Guarded(codec, size[o], shift=out_shift if o in "bqn" else 0) for o in "bqlno" if o in outputs}

    def p(o):
        return g[o].ptr if o in g else None

    def cap(o, entries):
        return entries if o in g else 0
    try:
        r = call(row_len=L, pad_base=pad_base, pad_qual=pad_qual, out_bases=p("b"), bases_cap=cap("b", n * L), out_quals=p("q"), quals_cap=cap("q", n * L),
                 out_lens=p("l"), lens_cap=cap("l", n), out_names=p("n"), names_cap=cap("n", nl), out_name_off=p("o"), off_cap=cap("o", n + 1))
        assert all(x.guards_intact() for x in g.values()), what + "a guard around an output buffer was written"
        body = {o: x.body() for o, x in g.items()}
        gB = np.frombuffer(body["b"], np.uint8).reshape(n, L) if "b" in g else None
        gQ = np.frombuffer(body["q"], np.uint8).reshape(n, L) if "q" in g else None
        gL = np.frombuffer(body["l"], np.int32) if "l" in g else None
        if gL is not None:
            assert np.array_equal(gL, e["lens"]), what + "lens differ"
        if "o" in g:
            want = np.concatenate([[0], np.cumsum([len(x) for x in e["names"]])]).astype(np.uint64)
            assert np.array_equal(np.frombuffer(body["o"], np.uint64), want), what + "name offsets differ"
        if "n" in g:
            assert body["n"] == b"".join(e["names"]), what + "the name blob differs"
        for got, rows, pad, kind in ((gB, e["bases"], pad_base, "base"), (gQ, e["quals"], pad_qual, "quality")):
            if got is not None and n:
                want = padded(rows, L, pad)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert not len(bad), what + rows_differ(kind, got, want, bad)
        return r, gB, gQ, gL, list(body.values())
    finally:
        for x in g.values():
            x.free()


def decode_rows_in_slices(codec, rfq: bytes, step: int, row_len: int, codes=False):
    """the streaming contract: `step` bytes at a time (has_header on the first call, final on the last, the unconsumed tail carried over);
    returns the concatenated (bases, quals, lens)"""
    outb, outq, outl = [], [], []
    pos, end, first = 0, min(step, len(rfq)), True
    while True:
        final = end == len(rfq)
        buf = rfq[pos:end]
        d = codec.dev_put(buf)
        try:
            q = codec.decode_rows(d, len(buf), has_header=first, final=final)
            n = q.n_rows
            if n:
                ob, oq, ol = codec.dev_put(b"\0" * (n * row_len)), codec.dev_put(b"\0" * (n * row_len)), codec.dev_put(b"\0" * (4 * n))
                r = codec.decode_rows(d, len(buf), row_len=row_len, codes=codes, has_header=first, final=final, d_bases=ob, bases_cap=n * row_len,
                                      d_quals=oq, quals_cap=n * row_len, d_lens=ol, lens_cap=n)
                assert (r.n_rows, r.consumed) == (q.n_rows, q.consumed)
                outb.append(np.frombuffer(codec.dev_get(ob, n * row_len), np.uint8).reshape(n, row_len))
                outq.append(np.frombuffer(codec.dev_get(oq, n * row_len), np.uint8).reshape(n, row_len))
                outl.append(np.frombuffer(codec.dev_get(ol, 4 * n), np.int32))
                for p in (ob, oq, ol):
                    codec.dev_free(p)
            consumed = q.consumed
        finally:
            codec.dev_free(d)
        first = False
        if final:
            break
        pos += consumed
        end = min(len(rfq), max(end, pos) + step)
    return np.concatenate(outb), np.concatenate(outq), np.concatenate(outl)


def run_hostile(codec, modes=((),), counts=None, seed=7, time_bound_s=60.0, good_every=1, tame=False):
    """_hostile's images and mutants through rfq_decode_rows: every call returns one of _hostile.ALLOWED or rows within the time bound, and after
    every `good_every`-th mutant the same context decodes the good image to the right rows.  Rows go into buffers sized for the good image (a mutant
    that claims more gets RFQ_E_NOSPACE).  Returns a summary dict."""
    from repaq_amd import RfqError
    summary = {"mutants": 0, "errors": {}, "decoded": 0, "slowest_s": 0.0, "slowest": None, "good_checks": 0}
    for label, img, _split, _want in H.images():
        n, ml, B, Q, lens = expected(img)
        L = (ml + 15) // 16 * 16 + 16                                         # (whole 16-byte groups: the kernel's vector path)
        want = expected(img, row_len=L)
        muts = H.mutants(img, seed, counts, tame)
        for mode in modes:
            for name, value in mode:
                codec.set_option(name, value)
            ob, oq, ol = codec.dev_put(b"\0" * (n * L)), codec.dev_put(b"\0" * (n * L)), codec.dev_put(b"\0" * (4 * n))
            try:
                for k, (mlabel, mimg, index) in enumerate(muts):
                    t0 = time.perf_counter()
                    d = codec.dev_put(mimg)
                    try:
                        codec.decode_rows(d, len(mimg), row_len=L, d_bases=ob, bases_cap=n * L, d_quals=oq, quals_cap=n * L, d_lens=ol, lens_cap=n,
                                          **({"chunk_off": index} if index else {}))
                        summary["decoded"] += 1; what = "decoded"
                    except RfqError as e:
                        oom = e.code == -2 and "out of memory" in e.message.lower()
                        assert e.code in H.ALLOWED or oom, "%s / %s / %s: error code %d (%s)" % (label, mode, mlabel, e.code, e.message)
                        what = "OOM" if oom else H.ALLOWED[e.code]
                        summary["errors"][what] = summary["errors"].get(what, 0) + 1
                    finally:
                        codec.dev_free(d)
                    dt = time.perf_counter() - t0
                    if dt > summary["slowest_s"]:
                        summary["slowest_s"], summary["slowest"] = round(dt, 3), "%s/%s" % (label, mlabel)
                    assert dt < time_bound_s, "%s / %s / %s took %.1f s" % (label, mode, mlabel, dt)
                    summary["mutants"] += 1
                    if k % good_every == 0 or k == len(muts) - 1:
                        d = codec.dev_put(img)
                        try:
                            r = codec.decode_rows(d, len(img), row_len=L, d_bases=ob, bases_cap=n * L, d_quals=oq, quals_cap=n * L, d_lens=ol, lens_cap=n)
                        finally:
                            codec.dev_free(d)
                        got = (np.frombuffer(codec.dev_get(ob, n * L), np.uint8).reshape(n, L), np.frombuffer(codec.dev_get(oq, n * L), np.uint8).reshape(n, L),
                               np.frombuffer(codec.dev_get(ol, 4 * n), np.int32))
                        assert r.n_rows == n and all(np.array_equal(x, y) for x, y in zip(got, want[2:])), \
                            "%s / %s: the good image decodes to other rows after mutant %s" % (label, mode, mlabel)
                        summary["good_checks"] += 1
            finally:
                for p in (ob, oq, ol):
                    codec.dev_free(p)
                for name, _ in mode:
                    codec.set_option(name, None)
    return summary
