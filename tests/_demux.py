"""Shared helpers of the rfq_demux_rows tests (tests/test_emu_demux.py on the SIMT interpreter, tests/test_gpu_demux.py on the MI355X).

Nothing expected comes from the code under test: the model is a plain Python loop over units, barcodes and positions, written from the rules of include/rfq_hip.h - a
position agrees when the row's byte is of class 0 .. 3 and equals the barcode's class, the distance is the count of the others, best / d1 / d2 come from the list
of distances, the verdict is two integer comparisons.  Every comparison is exact equality of every output array, of the counts and of every result field.  Every
output goes into a _rows.Guarded buffer of exactly the bytes the call may write, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R

FIELDS = ("n_units", "n_candidates", "n_assigned", "n_samples", "n_exact", "why_none", "why_ambig", "why_short", "why_combo", "bases_in", "bases_out")
OPTION = "RFQ_DEMUX"
PATHS = (None, "general")
E_ARG = -3
NONE, AMBIG, SHORT, COMBO, MASKED = 1, 2, 4, 8, 128

# ---------------------------------------------------------------- the model
ASCII_CLS = [4] * 256
CODE_CLS = [4] * 256
for _i, _b in enumerate(b"ACGT"):
    ASCII_CLS[_b] = ASCII_CLS[_b | 0x20] = CODE_CLS[_i] = _i


class Cfg:
    """the arguments of a call beside the rows: sets as lists of bytes, the sheet as a list of (i, j) or None"""
    def __init__(self, set1, set2=None, sheet=None, pairs=False, off1=0, off2=0, skip1=0, skip2=0, max_mm=1, min_delta=1):
        self.sets = [list(set1), list(set2) if set2 is not None else None]
        self.sheet, self.pairs, self.off, self.skip, self.max_mm, self.min_delta = sheet, pairs, (off1, off2), (skip1, skip2), max_mm, min_delta

    @property
    def n_samples(self):
        if self.sets[1] is None:
            return len(self.sets[0])
        return len(self.sheet) if self.sheet is not None else len(self.sets[0]) * len(self.sets[1])

    def kw(self):
        return dict(barcodes1=self.sets[0], barcodes2=self.sets[1], sheet=self.sheet, pairs=self.pairs, off1=self.off[0], off2=self.off[1], skip1=self.skip[0],
                    skip2=self.skip[1], max_mm=self.max_mm, min_delta=self.min_delta)


def row_match(row, l, bcs, off, max_mm, min_delta, CL, memo):
    """(best, d1, why bits) of one row against one set"""
    ln = len(bcs[0])
    if l < off + ln:
        return -1, 255, SHORT
    key = (bytes(row[off:off + ln]), id(bcs), max_mm, min_delta)
    if key in memo:
        return memo[key]
    ds = []
    for b in bcs:
        d = 0
        for j in range(ln):
            c = CL[row[off + j]]
            if c > 3 or c != ASCII_CLS[b[j]]:
                d += 1
        ds.append(d)
    d1 = min(ds); best = ds.index(d1)
    others = ds[:best] + ds[best + 1:]
    d2 = min(others) if others else ln + 1
    why = NONE if d1 > max_mm else (AMBIG if d2 - d1 < min_delta else 0)
    memo[key] = (best, d1, why)
    return memo[key]


def expected(B, lens, cfg, codes, cand=None):
    n = len(lens); nr = 2 if cfg.pairs else 1; U = n // nr; CL = CODE_CLS if codes else ASCII_CLS
    ns = cfg.n_samples
    table = {p: s for s, p in enumerate(map(tuple, cfg.sheet))} if cfg.sheet is not None else None
    sample = np.full(U, -1, np.int32); why = np.zeros(U, np.uint8); best = np.full(n, -1, np.int32); dist = np.full(n, 255, np.uint8)
    keep = np.zeros(n, np.uint8); start = np.zeros(n, np.int32); counts = np.zeros(ns + 1, np.uint64)
    s = dict.fromkeys(FIELDS, 0); s["n_units"] = U; s["n_samples"] = ns
    memo = {}
    rows = [bytes(r) for r in B]
    for u in range(U):
        g = [nr * u + i for i in range(nr)]
        if cand is not None and not all(cand[x] for x in g):
            why[u] = MASKED
            continue
        s["n_candidates"] += 1; s["bases_in"] += sum(int(lens[x]) for x in g)
        w = 0; bs = []; exact = True
        for i, x in enumerate(g):
            if cfg.sets[i] is None:
                continue
            b, d, bits = row_match(rows[x], int(lens[x]), cfg.sets[i], cfg.off[i], cfg.max_mm, cfg.min_delta, CL, memo)
            best[x] = b; dist[x] = d; w |= bits; bs.append(b); exact = exact and d == 0
        smp = -1
        if w == 0:
            if cfg.sets[1] is None:
                smp = bs[0]
            elif table is None:
                smp = bs[0] * len(cfg.sets[1]) + bs[1]
            else:
                smp = table.get((bs[0], bs[1]), -1)
                if smp < 0:
                    w = COMBO
        why[u] = w
        for bit, f in ((NONE, "why_none"), (AMBIG, "why_ambig"), (SHORT, "why_short"), (COMBO, "why_combo")):
            s[f] += 1 if w & bit else 0
        if w:
            counts[ns] += 1
            continue
        sample[u] = smp; counts[smp] += 1; s["n_assigned"] += 1; s["n_exact"] += 1 if exact else 0
        for i, x in enumerate(g):
            keep[x] = 1
            if cfg.sets[i] is not None:
                start[x] = min(int(lens[x]), cfg.off[i] + len(cfg.sets[i][0]) + cfg.skip[i])
            s["bases_out"] += int(lens[x]) - int(start[x])
    return dict(sample=sample, why=why, best=best, dist=dist, keep=keep, start=start, counts=counts, summary=s)


# ---------------------------------------------------------------- rows and calls
LETTERS = np.frombuffer(b"ACGT", np.uint8)
TO_CODE = bytes.maketrans(b"ACGTacgtN", b"\x00\x01\x02\x03\x00\x01\x02\x03\x04")


def rand_seq(rng, n):
    return LETTERS[rng.integers(0, 4, n)].tobytes()


def rows_of(seqs, L, codes=False, pad=None, lens=None):
    """(B, lens): the sequences (ASCII bytes; N is a base of class other) as rows of stride L, in code mode as codes; pad None: random bases behind the reads"""
    rng = np.random.default_rng(len(seqs) * 131 + L)
    B = LETTERS[rng.integers(0, 4, (len(seqs), L))] if pad is None else np.full((len(seqs), L), pad, np.uint8)
    for i, s in enumerate(seqs):
        B[i, :len(s)] = np.frombuffer(s, np.uint8)
    if codes:
        B = np.frombuffer(B.tobytes().translate(TO_CODE), np.uint8).reshape(B.shape).copy()
    return np.ascontiguousarray(B), (np.array([len(s) for s in seqs], np.int32) if lens is None else np.asarray(lens, np.int32))


def mutate(bc, pos, to=None):
    """the barcode with another base (or `to`) at pos"""
    b = bytearray(bc)
    b[pos] = to if to is not None else b"ACGT"[(b"ACGT".index(bytes([b[pos] & 0xDF])) + 1) % 4]
    return bytes(b)


def distinct_barcodes(rng, n, ln, min_dist=0):
    out = []
    while len(out) < n:
        c = rand_seq(rng, ln)
        if all(sum(x != y for x, y in zip(c, o)) >= max(min_dist, 1) for o in out):
            out.append(c)
    return out


def dev_rows(codec, B, lens, cand=None, shift=0):
    return W.DevRows(codec, B, None, lens, shift=shift, cand=(cand, np.uint8))


NAMES = dict(s="sample", w="why", b="best", d="dist", k="keep", t="start", c="counts")
DTYPES = dict(s=np.int32, w=np.uint8, b=np.int32, d=np.uint8, k=np.uint8, t=np.int32, c=np.uint64)
OUT_ARGS = dict(s="d_sample", w="d_why", b="d_best", d="d_dist", k="d_keep", t="d_start", c="d_counts")
ALL = "swbdktc"


def summary_of(r):
    return {f: int(getattr(r, f)) for f in FIELDS}


def run(codec, dev, cfg, codes=False, outputs=ALL):
    """one rfq_demux_rows into Guarded buffers of exactly the bytes the call may write; returns (dict of numpy outputs, summary dict, raw bytes of the outputs)"""
    n = dev.n; U = n // (2 if cfg.pairs else 1)
    sizes = dict(s=4 * U, w=U, b=4 * n, d=n, k=n, t=4 * n, c=8 * (cfg.n_samples + 1))
    g = {o: W.Guarded(codec, sizes[o]) for o in outputs}
    try:
        r = codec.demux_rows(*dev.adapter_args(), codes=codes, d_in=dev.cand, **cfg.kw(), **{OUT_ARGS[o]: g[o].ptr for o in outputs})
        assert all(x.guards_intact() for x in g.values()), "a guard around an output buffer was written"
        raw = {o: x.body() for o, x in g.items()}
        return {o: np.frombuffer(raw[o], DTYPES[o]) for o in outputs}, summary_of(r), raw
    finally:
        for x in g.values():
            x.free()


def compare(out, summ, e, what=""):
    for o, got in out.items():
        want = e[NAMES[o]]
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]; i = int(bad[0])
            raise AssertionError("%s %s differs in %d of %d entries, first %d: got %r, want %r" % (what, NAMES[o], len(bad), len(want), i, got[i], want[i]))
    assert summ == e["summary"], (what, {k: (summ[k], e["summary"][k]) for k in FIELDS if summ[k] != e["summary"][k]})


def check(codec, B, lens, cfg, codes=False, cand=None, shifts=(0,), paths=PATHS, outputs=ALL, what=""):
    """the call equals the model, at every shift and on every path, and the paths give equal bytes; returns the model's result"""
    e = expected(B, lens, cfg, codes, cand)
    for shift in shifts:
        dev = dev_rows(codec, B, lens, cand, shift)
        try:
            raws = []
            for path in paths:
                codec.set_option(OPTION, path)
                out, summ, raw = run(codec, dev, cfg, codes, outputs)
                compare(out, summ, e, "%s shift %d option %s:" % (what, shift, path or "default"))
                raws.append(raw)
            assert all(r == raws[0] for r in raws), what + " the formulations give different bytes"
        finally:
            codec.set_option(OPTION, None)
            dev.free()
    return e


# ---------------------------------------------------------------- test 1: every barcode at every distance
PLANT_LENS = (1, 8, 16, 17, 32)


def check_every_distance(codec, ln):
    """7 barcodes (4 of length 1: there are no more) planted exact, with one mismatch at every position, with an N at every position and in lower case, as ASCII
    and as codes"""
    rng = np.random.default_rng(100 + ln)
    bcs = distinct_barcodes(rng, 7 if ln > 1 else 4, ln, min_dist=min(3, ln))
    off = 3
    seqs = []
    for b in bcs:
        seqs.append(b)
        seqs += [mutate(b, p) for p in range(ln)] + [mutate(b, p, ord("N")) for p in range(ln)]
        seqs.append(b.lower())
    tail = rand_seq(rng, 9)
    seqs = [rand_seq(rng, off) + s + tail for s in seqs]
    for codes in (False, True):
        B, lens = rows_of(seqs, off + ln + 12, codes)
        for max_mm in (0, 1):
            e = check(codec, B, lens, Cfg(bcs, off1=off, skip1=2, max_mm=max_mm), codes, what="len %d codes %d max_mm %d" % (ln, codes, max_mm))
            s = e["summary"]
            assert s["n_exact"] >= len(bcs) and (ln == 1 or (s["why_none"] > 0) == (max_mm == 0)) and int(e["dist"].max()) >= 1


# ---------------------------------------------------------------- test 2: window seams
SEAM_OFFS = (0, 1, 15, 16, 17, 31, 40)
SEAM_LENS = (1, 15, 16, 17, 32)


def check_seams(codec, off):
    rng = np.random.default_rng(200 + off)
    for ln in SEAM_LENS:
        bcs = distinct_barcodes(rng, 5 if ln > 1 else 4, ln, min_dist=min(3, ln))
        for L in sorted({ln + off, 48, 50, 150, 160}):
            if L < off + ln:
                continue
            seqs, lens = [], []
            for k, b in enumerate(bcs):
                for s, l in ((b, off + ln), (mutate(b, ln - 1), off + ln), (mutate(b, 0), L), (b, off + ln - 1), (b, 0), (mutate(b, ln // 2, ord("N")), min(L, off + ln + 3))):
                    seqs.append((rand_seq(rng, off) + s + rand_seq(rng, L))[:L]); lens.append(l)
            seqs.append((rand_seq(rng, off) + bcs[-1])[:L]); lens.append(off + ln)       # the last row ends exactly at the buffer's end when L == off + ln
            B, lens = rows_of(seqs, L, lens=lens)
            for skip in (0, 5):
                e = check(codec, B, lens, Cfg(bcs, off1=off, skip1=skip), shifts=(0, 1, 5), what="off %d len %d L %d skip %d" % (off, ln, L, skip))
                assert e["summary"]["why_short"] == (2 if off + ln > 0 else 1) * len(bcs) and e["summary"]["n_assigned"] >= len(bcs)
                assert skip == 0 or L == off + ln or int(e["start"].max()) == min(L, off + ln + skip)


# ---------------------------------------------------------------- test 3: ties and deltas
def check_ties(codec):
    rng = np.random.default_rng(300)
    ln = 8
    a = rand_seq(rng, ln); far = mutate(mutate(mutate(mutate(mutate(a, 0), 1), 2), 3), 4)
    for h in (1, 2, 3):
        b = a
        for p in range(h):
            b = mutate(b, ln - 1 - p)
        mids = [a, b]
        x = a
        for p in range(h):                                                   # the reads on the way from a to b: 0 .. h of b's bases
            x = mutate(x, ln - 1 - p, b[ln - 1 - p]); mids.append(x)
        mids += [mutate(a, 0), mutate(b, 0), mutate(mutate(a, 0), 1), far, mutate(far, 7, ord("N"))]
        B, lens = rows_of([m + rand_seq(rng, 4) for m in mids], 16)
        for order in ([a, b, far], [b, a, far], [far, b, a]):               # the runner-up before and after the best
            for max_mm in range(4):
                for min_delta in range(4):
                    e = check(codec, B, lens, Cfg(order, max_mm=max_mm, min_delta=min_delta), what="ties h %d mm %d delta %d" % (h, max_mm, min_delta))
                    assert min_delta or e["summary"]["why_ambig"] == 0
        # one barcode: d2 = len + 1, so every delta up to len + 1 - d1 passes
        for min_delta in (0, 1, 8, 9, 33):
            e = check(codec, B, lens, Cfg([a], max_mm=3, min_delta=min_delta), what="one barcode delta %d" % min_delta)
            near = sum(1 for m in mids if sum(x != y for x, y in zip(m, a)) <= min(3, 9 - min_delta))      # d1 <= max_mm and 9 - d1 >= min_delta
            assert e["summary"]["n_assigned"] == near and (near > 0) == (min_delta <= 9)
    # 4096 barcodes of 8 bases (what the LDS holds of one set at two words; here one): the hit is the first and the last
    digits = lambda v: bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(8))
    many = [digits(v * 16 + (v % 7)) for v in range(4096)]
    assert len(set(many)) == 4096
    B, lens = rows_of([many[0], many[4095], mutate(many[0], 7), mutate(many[4095], 0), mutate(many[2000], 3, ord("N")), many[1234].lower()], 8)
    for max_mm, min_delta in ((0, 1), (1, 0), (1, 1)):
        e = check(codec, B, lens, Cfg(many, max_mm=max_mm, min_delta=min_delta), what="4096 barcodes")
        assert list(e["best"][:2]) == [0, 4095] and list(e["sample"][:2]) == [0, 4095]


# ---------------------------------------------------------------- test 4: pairs
def pair_rows(rng, set1, set2, off, L, sheet=None):
    """(seqs, lens, cand) of units that show every reason alone: exact pairs of every listed and some unlisted combinations, one mismatch, NONE in R1 / R2, AMBIG,
    SHORT in R1 / R2, a masked mate"""
    l1, l2 = len(set1[0]), len(set2[0]) if set2 else 0
    def r1(bc, l=None):
        s = rand_seq(rng, off[0]) + bc + rand_seq(rng, 20); return s[:L], (len(s[:L]) if l is None else l)
    def r2(bc, l=None):
        s = rand_seq(rng, off[1]) + bc + rand_seq(rng, 17); return s[:L], (len(s[:L]) if l is None else l)
    units = []
    for i, a in enumerate(set1):
        for j, b in enumerate(set2 or [b""]):
            units.append((r1(a), r2(b)))
    a, b = set1[0], (set2 or [b""])[0]
    junk1 = bytes(b"ACGT"[(b"ACGT".index(bytes([c])) + 2) % 4] for c in a)
    units.append((r1(mutate(a, l1 - 1)), r2(b)))
    units.append((r1(junk1), r2(b)))                                         # NONE alone (R1)
    units.append((r1(a, off[0] + l1 - 1), r2(b)))                            # SHORT alone (R1)
    units.append((r1(a, 0), r2(b, 0)))
    if set2:
        junk2 = bytes(b"ACGT"[(b"ACGT".index(bytes([c])) + 2) % 4] for c in b)
        units.append((r1(a), r2(junk2)))                                     # NONE alone (R2)
        units.append((r1(a), r2(b, off[1] + l2 - 1)))                        # SHORT alone (R2)
        units.append((r1(a), r2(mutate(b, 0, ord("N")))))
    seqs = [s for u in units for s, _ in u]; lens = [l for u in units for _, l in u]
    return seqs, lens


def check_pairs(codec):
    rng = np.random.default_rng(400)
    set1 = distinct_barcodes(rng, 6, 8, min_dist=4); set2 = distinct_barcodes(rng, 5, 17, min_dist=5)
    amb = mutate(set1[0], 2); set1a = set1 + [mutate(amb, 5)]                # set1a[6] is 2 from set1[0]: `amb` is 1 from both -> AMBIG
    off = (2, 19); L = 64
    every = [(i, j) for i in range(len(set1a)) for j in range(len(set2))]
    sheet = [(0, 0)] + [every[k] for k in rng.permutation(len(every))[:len(every) // 3] if every[k] != (0, 0)]      # a third of the pairs; (0, 0) is one of them
    for codes in (False, True):
        for s2, sh in ((set2, None), (set2, sheet), (None, None)):
            seqs, lens = pair_rows(rng, set1a, s2, off, L)
            seqs += [(rand_seq(rng, off[0]) + amb + rand_seq(rng, 20))[:L], (rand_seq(rng, off[1]) + (s2 or [b""])[0] + rand_seq(rng, 9))[:L]]; lens += [L, L]
            B, lens = rows_of(seqs, L, codes, lens=lens)
            n = len(lens)
            cfg = Cfg(set1a, s2, sh, pairs=True, off1=off[0], off2=off[1] if s2 else 0, skip1=1, skip2=3 if s2 else 0)
            e = check(codec, B, lens, cfg, codes, what="pairs codes %d set2 %d sheet %d" % (codes, s2 is not None, sh is not None))
            why = e["why"]
            for bit in (NONE, AMBIG, SHORT) + ((COMBO,) if sh else ()):
                assert int((why == bit).sum()) > 0, "the reason %d does not occur alone" % bit
            assert e["summary"]["n_exact"] > 0 and e["summary"]["n_exact"] < e["summary"]["n_assigned"]
            if s2 is None:                                                   # the odd rows have no set
                assert (e["best"][1::2] == -1).all() and (e["dist"][1::2] == 255).all() and (e["start"][1::2] == 0).all()
            # d_in masks one mate of a few units: MASKED alone, not counted
            cand = np.ones(n, np.uint8); cand[1] = 0; cand[6] = 0; cand[n - 1] = 0
            m = check(codec, B, lens, cfg, codes, cand=cand, what="masked mates")
            assert list(m["why"][[0, 3, n // 2 - 1]]) == [MASKED] * 3 and m["summary"]["n_candidates"] == n // 2 - 3
            assert int(m["counts"].sum()) == n // 2 - 3
            # fewer outputs than all
            check(codec, B, lens, cfg, codes, outputs="kt", paths=(None,), what="two outputs")
            check(codec, B, lens, cfg, codes, outputs="", paths=(None,), what="no outputs")


# ---------------------------------------------------------------- test 5: the walk
WALK_IDS = W.WALK_IDS


def walk_rows(rng, n, L, bcs, off):
    ln = len(bcs[0])
    seqs = []
    for i in range(n):
        l = int(rng.integers(0, min(L, 60) + 1)) if i % 4 else min(L, off + ln + 10)
        s = bytearray(rand_seq(rng, l))
        if i % 3 and l >= off + ln:
            s[off:off + ln] = bcs[int(rng.integers(0, len(bcs)))]
        seqs.append(bytes(s))
    return seqs


def check_walk(codec, label):
    """unit counts around a wave and a workgroup's step (a lane takes a unit: 64 and 256) beside the family's own, rows and pairs"""
    L, path, counts = W.walk_case(label, 1)
    counts = sorted(set(counts) | {63, 64, 65, 255, 256, 257, 513})
    rng = np.random.default_rng(500 + L)
    set1 = distinct_barcodes(rng, 12, 9, min_dist=3); set2 = distinct_barcodes(rng, 3, 6, min_dist=3)
    for U in counts:
        for pairs in (False, True):
            n = (2 if pairs else 1) * U
            B, lens = rows_of(walk_rows(rng, n, L, set1 if not pairs else set1[:5], 4), L, pad=ord("A"))
            B[:, L - 9:] = np.frombuffer(set1[0], np.uint8)                    # (bytes in the row's last group, none of them inside a read)
            cfg = Cfg(set1, off1=4) if not pairs else Cfg(set1[:5], set2, pairs=True, off1=4, off2=1)
            if pairs:
                for r in range(3, n, 6):                                      # (their mates are rows 2, 8, ..: planted where long enough)
                    B[r, 1:7] = np.frombuffer(set2[r % 3], np.uint8); lens[r] = max(lens[r], 7)
            e = check(codec, B, lens, cfg, shifts=(n % 16,), paths=(path,), what="walk L %d units %d pairs %d" % (L, U, pairs))
            assert U < 63 or e["summary"]["n_assigned"] >= 1


def check_walk_bad_length(codec):
    """a bad length in the last row, one unit behind a workgroup's step: the refusal names it"""
    from repaq_amd import RfqError
    rng = np.random.default_rng(55)
    bcs = distinct_barcodes(rng, 4, 8)
    for L in (24, 272):
        n = 257
        B, lens = rows_of([rand_seq(rng, 20)] * n, L)
        lens[n - 1] = L + 1
        dev = dev_rows(codec, B, lens)
        try:
            for path in PATHS:
                codec.set_option(OPTION, path)
                with R.pytest_raises(RfqError) as ei:
                    run(codec, dev, Cfg(bcs))
                assert ei.value.code == E_ARG and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
        finally:
            codec.set_option(OPTION, None)
            dev.free()


def check_counts_paths(codec, cells):
    """n_samples + 1 = 8192 (the LDS table's last size) and 8193 (global atomics): 128 x 64 barcodes, a sheet of 8191 / 8192 pairs"""
    rng = np.random.default_rng(560 + cells)
    digits = lambda v, ln: bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(ln))
    set1 = [digits(v * 5 + 1, 6) for v in range(128)]; set2 = [digits(v * 3 + 2, 5) for v in range(64)]
    every = [(i, j) for i in range(128) for j in range(64)]
    sheet = [every[k] for k in rng.permutation(8192)[:cells - 1]]
    picks = [sheet[0], sheet[-1], sheet[len(sheet) // 2]] + [every[int(k)] for k in rng.integers(0, 8192, 40)]
    seqs = []
    for u in range(700):
        i, j = picks[u % len(picks)]
        seqs += [set1[i] + rand_seq(rng, 6), (set2[j] if u % 11 else mutate(set2[j], 4, ord("N"))) + rand_seq(rng, 3)]
    B, lens = rows_of(seqs, 12)
    cfg = Cfg(set1, set2, sheet, pairs=True, max_mm=0)
    e = check(codec, B, lens, cfg, what="%d count cells" % cells)
    assert cfg.n_samples + 1 == cells and e["summary"]["n_assigned"] > 300 and int(e["counts"][-1]) > 0 and int(e["counts"][cfg.n_samples - 1]) > 0


def check_many_rows(codec, n=300_006):
    """300 006 short rows built from a few hundred distinct ones: more than the 262 144 units one step of the capped grid takes on 256 compute units (4 workgroups
    each, 256 lanes) - the interpreter reports 4 compute units: 4096 units a step -, so workgroups take several steps, and the last workgroup is part empty"""
    rng = np.random.default_rng(570)
    bcs = distinct_barcodes(rng, 24, 8, min_dist=3)
    pool = walk_rows(rng, 300, 16, bcs, 2)
    Bp, lp = rows_of(pool, 16)
    pick = rng.integers(0, 300, n)
    B, lens = np.ascontiguousarray(Bp[pick]), lp[pick].copy()
    cfg = Cfg(bcs, off1=2)
    ep = expected(Bp, lp, cfg, False)                                         # the model on the distinct rows, gathered
    e = {k: ep[k][pick] for k in ("sample", "why", "best", "dist", "keep", "start")}
    dev = dev_rows(codec, B, lens)
    try:
        out, summ, _ = run(codec, dev, cfg)
    finally:
        dev.free()
    for o in "swbdkt":
        assert np.array_equal(out[o], e[NAMES[o]]), NAMES[o]
    assert np.array_equal(out["c"][:24], np.bincount(e["sample"][e["sample"] >= 0], minlength=24).astype(np.uint64)) and int(out["c"][24]) == int((e["sample"] < 0).sum())
    hit = e["sample"] >= 0
    want = dict(n_units=n, n_candidates=n, n_assigned=int(hit.sum()), n_samples=24, n_exact=int((hit & (e["dist"] == 0)).sum()), why_none=int((e["why"] & NONE != 0).sum()),
                why_ambig=int((e["why"] & AMBIG != 0).sum()), why_short=int((e["why"] & SHORT != 0).sum()), why_combo=0, bases_in=int(lens.sum()),
                bases_out=int((lens - e["start"])[hit].sum()))
    assert summ == want, (summ, want)


def check_lds_max(codec):
    """the most LDS a call can ask for: 4096 + 256 barcodes of two words (n1 * n2 = 2^20) and 8192 count cells, 34 + 32 KiB"""
    rng = np.random.default_rng(580)
    digits = lambda v, ln: bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(ln))
    set1 = [digits(v * 1021 + 5, 17) for v in range(4096)]; set2 = [digits(v * 77 + 9, 20) for v in range(256)]
    assert len(set(set1)) == 4096 and len(set(set2)) == 256
    listed = sorted(int(k) for k in rng.permutation(1 << 20)[:8191])
    sheet = [(k >> 8, k & 255) for k in listed]
    picks = [sheet[0], sheet[-1], sheet[4000], (4095, 255), (0, 0), (4095, 0)]
    seqs = []
    for u in range(24):
        i, j = picks[u % len(picks)]
        seqs += [(set1[i] if u % 5 else mutate(set1[i], 16)) + rand_seq(rng, 3), b"AC" + (set2[j] if u % 7 else mutate(set2[j], 19, ord("N"))) + rand_seq(rng, 2)]
    B, lens = rows_of(seqs, 24)
    cfg = Cfg(set1, set2, sheet, pairs=True, off2=2)
    e = check(codec, B, lens, cfg, what="the largest LDS")
    assert cfg.n_samples + 1 == 8192 and e["summary"]["n_assigned"] >= 8 and int(e["counts"][8190]) > 0 and int(e["counts"][0]) > 0


# ---------------------------------------------------------------- test 6: the switch
def check_option(codec, reset):
    from repaq_amd import RfqError
    assert OPTION in codec.option_names() and codec.get_option(OPTION) == ""
    codec.set_option(OPTION, "general")
    assert codec.get_option(OPTION) == "general"
    reset(codec)
    assert codec.get_option(OPTION) == ""
    for bad in ("staged", "collide", "General", "1"):
        with R.pytest_raises(RfqError):
            codec.set_option(OPTION, bad)
    assert codec.get_option(OPTION) == ""


# ---------------------------------------------------------------- test 7: refusals
def _good(codec):
    """what every refusal is followed by, on the same context: a call that gives the model's result"""
    rng = np.random.default_rng(9)
    s1 = distinct_barcodes(rng, 3, 6, min_dist=3); s2 = distinct_barcodes(rng, 2, 18, min_dist=3)
    seqs = [s1[1] + rand_seq(rng, 20), s2[0] + rand_seq(rng, 5), mutate(s1[2], 0) + rand_seq(rng, 20), s2[1] + rand_seq(rng, 5), rand_seq(rng, 30), s2[1]]
    B, lens = rows_of(seqs, 40)
    check(codec, B, lens, Cfg(s1, s2, [(1, 0), (2, 1)], pairs=True), paths=(None,), what="after a refusal")


def check_host_refusals(codec):
    from repaq_amd import RfqError
    rng = np.random.default_rng(61)
    s1 = distinct_barcodes(rng, 4, 8, min_dist=2); s2 = distinct_barcodes(rng, 3, 6, min_dist=2)
    B, lens = rows_of([rand_seq(rng, 30) for _ in range(12)], 32)
    n, L = B.shape
    dev = dev_rows(codec, B, lens, np.ones(n, np.uint8))
    buf = codec.dev_put(b"\0" * 16384); b = buf.value
    try:
        rows = dev.adapter_args()

        def at(p, k):
            return C.c_void_p(p.value + k)
        D = codec.demux_rows
        P = dict(pairs=True, barcodes2=s2)
        big = [bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(6)) for v in range(2048)]
        sheet_ptr = (C.c_int32 * 4)(0, 0, 1, 1)
        calls = (("pairs takes rows in pairs", lambda: D(n - 1, L, dev.bases, dev.lens, s1, pairs=True)),
                 ("pairs must be 0 or 1", lambda: D(*rows, s1, raw=dict(pairs=2))),
                 ("are for pairs", lambda: D(*rows, s1, barcodes2=s2)),
                 ("are for pairs", lambda: D(*rows, s1, raw=dict(h_pairs=sheet_ptr, n_samples=2))),
                 ("are for pairs", lambda: D(*rows, s1, skip2=1)),
                 ("are for pairs", lambda: D(*rows, s1, off2=1)),
                 ("h_pairs needs set 2", lambda: D(*rows, s1, pairs=True, sheet=[(0, 0)])),
                 ("no set 1", lambda: D(*rows, None)),
                 ("no set 1", lambda: D(*rows, None, **P)),
                 ("null h_bc1", lambda: D(*rows, s1, raw=dict(h_bc1=None))),
                 ("null h_bc2", lambda: D(*rows, s1, pairs=True, raw=dict(n2=3, len2=6))),
                 ("set 1: the number of barcodes", lambda: D(*rows, s1, raw=dict(n1=0))),
                 ("set 1: the number of barcodes", lambda: D(*rows, s1, raw=dict(n1=4097))),
                 ("set 2: the number of barcodes", lambda: D(*rows, s1, **P, raw=dict(n2=0))),
                 ("set 1: the barcode length", lambda: D(*rows, s1, raw=dict(len1=0))),
                 ("set 1: the barcode length", lambda: D(*rows, [x * 5 for x in s1][:2], raw=dict(len1=33))),
                 ("set 2: the barcode length", lambda: D(*rows, s1, **P, raw=dict(len2=0))),
                 ("n1 * n2 is at most 2^20", lambda: D(*rows, big, pairs=True, barcodes2=big[:513])),
                 ("max_mm is at most 32", lambda: D(*rows, s1, max_mm=33)),
                 ("max_mm is at most 32", lambda: D(*rows, s1, min_delta=34)),
                 ("n_samples must be", lambda: D(*rows, s1, **P, sheet=[])),
                 ("n_samples must be", lambda: D(*rows, s1, **P, sheet=[(0, 0)], raw=dict(n_samples=65537))),
                 ("not one of ACGTacgt (0x4e at 3)", lambda: D(*rows, [s1[0], mutate(s1[1], 3, ord("N"))])),
                 ("set 2: barcode 2 holds a byte", lambda: D(*rows, s1, pairs=True, barcodes2=[s2[0], s2[1], b"ACG\x00AC"])),
                 ("set 1: barcodes 1 and 3 are equal", lambda: D(*rows, [s1[0], s1[1], s1[2], s1[1].lower()])),
                 ("set 2: barcodes 0 and 2 are equal", lambda: D(*rows, s1, pairs=True, barcodes2=[s2[0], s2[1], s2[0]])),
                 ("pair 1 is (4, 0)", lambda: D(*rows, s1, **P, sheet=[(0, 0), (4, 0)])),
                 ("pair 0 is (0, 3)", lambda: D(*rows, s1, **P, sheet=[(0, 3)])),
                 ("pair 0 is (-1, 0)", lambda: D(*rows, s1, **P, sheet=[(-1, 0)])),
                 ("lists the pair (1, 2) twice", lambda: D(*rows, s1, **P, sheet=[(1, 2), (0, 0), (1, 2)])),
                 ("set 1: off + len + skip", lambda: D(*rows, s1, off1=0x7FFFFFFF - 8, skip1=1)),
                 ("set 1: off + len + skip", lambda: D(*rows, s1, off1=0xFFFFFFFF, skip1=0xFFFFFFFF)),
                 ("set 2: off + len + skip", lambda: D(*rows, s1, **P, skip2=0x7FFFFFFF)),
                 ("bad base_mode", lambda: D(*rows, s1, base_mode=7)),
                 ("row_len must be >= 1", lambda: D(n, 0, dev.bases, dev.lens, s1)),
                 ("null d_lens / d_bases", lambda: D(n, L, None, dev.lens, s1)),
                 ("null d_lens / d_bases", lambda: D(n, L, dev.bases, None, s1)),
                 ("4-byte aligned", lambda: D(n, L, dev.bases, at(dev.lens, 2), s1)),
                 ("4-byte aligned", lambda: D(*rows, s1, d_sample=C.c_void_p(b + 2))),
                 ("4-byte aligned", lambda: D(*rows, s1, d_best=C.c_void_p(b + 1))),
                 ("4-byte aligned", lambda: D(*rows, s1, d_start=C.c_void_p(b + 3))),
                 ("d_counts must be 8-byte aligned", lambda: D(*rows, s1, d_counts=C.c_void_p(b + 4))),
                 ("d_keep overlaps the input rows->d_bases", lambda: D(*rows, s1, d_keep=at(dev.bases, n * L - 1))),
                 ("d_keep overlaps the input d_in", lambda: D(*rows, s1, d_in=dev.cand, d_keep=dev.cand)),
                 ("d_start overlaps the input rows->d_lens", lambda: D(*rows, s1, d_start=dev.lens)),
                 ("d_counts overlaps the input d_in", lambda: D(*rows, s1, d_in=dev.cand, d_counts=at(dev.cand, 8 - dev.cand.value % 8))),
                 ("d_sample overlaps the output d_why", lambda: D(*rows, s1, d_sample=C.c_void_p(b), d_why=C.c_void_p(b + 4 * n - 1))),
                 ("d_best overlaps the output d_start", lambda: D(*rows, s1, d_best=C.c_void_p(b), d_start=C.c_void_p(b + 4))),
                 ("d_dist overlaps the output d_counts", lambda: D(*rows, s1, d_dist=C.c_void_p(b + 8 * 4), d_counts=C.c_void_p(b))),
                 ("too many rows", lambda: D(1 << 31, 1, dev.bases, dev.lens, s1)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == E_ARG and what in ei.value.message, (what, ei.value)
            _good(codec)
        # (outputs of the caller's own that lie on nothing are taken; the quality rows are not an input; no rows at all fill n_samples and zero the counts)
        assert D(*rows, s1, d_best=C.c_void_p(b), d_start=C.c_void_p(b + 1024), d_keep=C.c_void_p(b + 4096)).n_units == n
        g = W.Guarded(codec, 8 * 13)
        try:
            r = summary_of(D(0, 0, None, None, s1, **P, d_counts=g.ptr))
            assert r == dict(dict.fromkeys(FIELDS, 0), n_samples=12) and g.guards_intact() and g.body() == b"\0" * (8 * 13)
        finally:
            g.free()
    finally:
        dev.free(); codec.dev_free(buf)


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "last", "pair_r1", "pair_r2")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    rng = np.random.default_rng(63)
    s1 = distinct_barcodes(rng, 5, 8); s2 = distinct_barcodes(rng, 3, 20)
    for L, n in ((24, 300), (300, 10), (1100, 6)):
        B = np.frombuffer(rand_seq(rng, n * L), np.uint8).reshape(n, L); lens = rng.integers(0, L + 1, n).astype(np.int32)
        pairs = where.startswith("pair")
        row = dict(first=0, last=n - 1, pair_r1=n // 2 & ~1, pair_r2=(n // 2 & ~1) + 1)[where]
        lens[row] = -1 if value == "negative" else L + 1
        cfg = Cfg(s1, s2, pairs=True, off2=3) if pairs else Cfg(s1)
        for cand in (None, (np.arange(n) != row).astype(np.uint8)):          # (every row is judged, candidate or not)
            dev = dev_rows(codec, B, lens, cand, shift=1)
            try:
                for path in PATHS:
                    codec.set_option(OPTION, path)
                    for outputs in ("", ALL):
                        with R.pytest_raises(RfqError) as ei:
                            run(codec, dev, cfg, outputs=outputs)
                        assert ei.value.code == E_ARG and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                    codec.set_option(OPTION, None)
                _good(codec)
            finally:
                codec.set_option(OPTION, None)
                dev.free()
    # two bad rows: the first is named
    lens = np.full(n, L, np.int32); lens[1] = -5; lens[4] = L + 1
    dev = dev_rows(codec, B, lens)
    try:
        with R.pytest_raises(RfqError) as ei:
            run(codec, dev, Cfg(s1))
        assert "first such row: 1)" in ei.value.message
    finally:
        dev.free()
    _good(codec)


# ---------------------------------------------------------------- test 8: state
def check_state(codec):
    """a demux call between two calls of each of the other kinds of call leaves their results unchanged (every kind is compared with its own host reference inside
    the call, and with what it gave first); a small set follows a large one and the other way round: the scratch only grows, nothing of the larger set is seen"""
    import _history as Hs
    import _kmers as K
    import _profile as P
    import _screen as S
    calls = Hs.calls()
    for kind in Hs.CALL_KINDS:
        first = getattr(calls, kind)(codec)
        _good(codec)
        assert getattr(calls, kind)(codec) == first, "a demux call changed what %s gives" % kind
    for good in (S._good, K._good, P._good):
        good(codec); _good(codec); good(codec)
    rng = np.random.default_rng(800)
    digits = lambda v, ln: bytes(b"ACGT"[(v >> (2 * j)) & 3] for j in range(ln))
    large1 = [digits(v * 9 + 4, 20) for v in range(1500)]; large2 = [digits(v * 7 + 1, 18) for v in range(600)]
    small = distinct_barcodes(rng, 2, 5, min_dist=2)
    seqs_l = [large1[7] + rand_seq(rng, 3), large2[599] + rand_seq(rng, 3), large1[1499] + b"AC", mutate(large2[0], 17) + b"GT", rand_seq(rng, 23), large2[3]]
    seqs_s = [small[0] + rand_seq(rng, 9), small[1], mutate(small[1], 4), rand_seq(rng, 5)]
    Bl, ll = rows_of(seqs_l, 24); Bs, ls = rows_of(seqs_s, 16)
    cl = Cfg(large1, large2, [(7, 599), (1499, 0), (3, 3)], pairs=True); cs = Cfg(small)
    for B, lens, cfg in ((Bs, ls, cs), (Bl, ll, cl), (Bs, ls, cs), (Bl, ll, cl)):
        e = check(codec, B, lens, cfg, what="small and large sets in turn")
        assert e["summary"]["n_assigned"] >= 2


# ---------------------------------------------------------------- test 9: composition with tensors
def compose_text(pairs=60, seed=14):
    """two paired FASTQ texts with inline barcodes (R1: 2 bases, an 8-base barcode, a linker base; R2: a 6-base barcode) and the sets and sheet they were made from"""
    rng = np.random.default_rng(seed)
    set1 = distinct_barcodes(rng, 4, 8, min_dist=3); set2 = distinct_barcodes(rng, 3, 6, min_dist=3)
    sheet = [(0, 0), (1, 1), (2, 2), (3, 0), (0, 2)]
    t1, t2 = [], []
    for p in range(pairs):
        i, j = sheet[p % 5] if p % 7 else (1, 2)                              # every seventh pair hops
        b1, b2 = set1[i], set2[j]
        if p % 5 == 1:
            b1 = mutate(b1, p % 8)
        if p % 11 == 3:
            b1 = rand_seq(rng, 8)
        if p % 13 == 4:
            b2 = mutate(b2, 2, ord("N"))
        s1 = rand_seq(rng, 2) + b1 + b"T" + rand_seq(rng, int(rng.integers(1, 40))); s2 = b2 + rand_seq(rng, int(rng.integers(1, 40)))
        if p % 17 == 5:
            s1 = s1[:7]
        if p % 19 == 6:
            s1 = s1[:11]                                                      # prefix, barcode and linker are the whole read: nothing is left of it where it is assigned
        q1 = bytes(b"F:,#5"[int(x)] for x in rng.integers(0, 5, len(s1))); q2 = bytes(b"F:,#5"[int(x)] for x in rng.integers(0, 5, len(s2)))
        t1.append(b"@p%d/1\n%s\n+\n%s\n" % (p, s1, q1)); t2.append(b"@p%d/2\n%s\n+\n%s\n" % (p, s2, q2))
    return (t1, t2), set1, set2, sheet


COMPOSE = dict(off1=2, skip1=1, off2=0, skip2=0, max_mm=1, min_delta=1)


def compose_expected(t1, t2, set1, set2, sheet):
    """per sample and for the unassigned bin (last) the two texts the host model leaves: the barcode, the prefix and the linker cut off the assigned reads; a pair
    one of whose reads has no base left is in no bin (select_rows' min_len = 1) - their number comes back too"""
    def rec(t):
        name, s, _, q = t.split(b"\n")[:4]
        return name, s, q
    seqs = []
    for a, b in zip(t1, t2):
        seqs += [rec(a)[1], rec(b)[1]]
    L = max(len(s) for s in seqs)
    B, lens = rows_of(seqs, L, pad=255)
    cfg = Cfg(set1, set2, sheet, pairs=True, **COMPOSE)
    e = expected(B, lens, cfg, False)
    out = [[b"", b""] for _ in range(len(sheet) + 1)]
    e["dropped"] = 0
    for u, (a, b) in enumerate(zip(t1, t2)):
        k = int(e["sample"][u]) if e["sample"][u] >= 0 else len(sheet)
        if any(int(lens[2 * u + m]) - int(e["start"][2 * u + m]) < 1 for m in (0, 1)):
            e["dropped"] += 1
            continue
        for m, t in enumerate((a, b)):
            name, s, q = rec(t); st = int(e["start"][2 * u + m])
            out[k][m] += b"%s\n%s\n+\n%s\n" % (name, s[st:], q[st:])
    return out, e
