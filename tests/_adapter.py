"""Shared helpers of the rfq_adapter_rows tests (tests/test_emu_adapter.py on the SIMT interpreter, tests/test_gpu_adapter.py on the MI355X).

Nothing expected comes from the code under test: overlap_of() and adapter_cut() restate the rules of include/rfq_hip.h as plain loops over the shifts and the
positions (one numpy slice compare per shift), expected() calls them per pair / per row and adds up the summary and the histogram.  Every output goes into a
_rows.Guarded buffer of exactly its size (0xA5 all over: the histogram starts as garbage), and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W

BY_OVERLAP, BY_ADAPTER = 1, 2
DEFAULTS = dict(pairs=False, min_overlap=0, max_diff=0, max_diff_pct=0, adapter1=None, adapter2=None, adapter_min=0, adapter_mm_per=0, hist_len=0)
FIELDS = ("n_rows", "n_pairs", "pairs_found", "rows_cut", "rows_cut_overlap", "rows_cut_adapter", "bases_in", "bases_out")
SHIFTS = (0, 1, 7, 15)
PATHS = (None, "general")
AD1, AD2 = b"AGATCGGAAGAGC", b"CTGTCTCTTATAC"

ASCII_CLASS = np.full(256, 4, np.uint8)
for _i, _b in enumerate(b"ACGT"):
    ASCII_CLASS[_b] = _i; ASCII_CLASS[_b + 32] = _i


def crit(**kw):
    c = dict(DEFAULTS); c.update(kw)
    assert set(c) == set(DEFAULTS), sorted(set(c) - set(DEFAULTS))
    return c


def classes(b, codes):
    """0 .. 3 = A C G T, 4 = other, of an array of base bytes"""
    b = np.asarray(b, np.uint8)
    return np.where(b < 4, b, 4).astype(np.uint8) if codes else ASCII_CLASS[b]


def overlap_of(x, r2, c):
    """(insert, diff) of one pair: x, r2 the classes of R1 and R2 (their lengths are the reads' lengths); (-1, 0) when no shift is acceptable"""
    l1, l2 = len(x), len(r2)
    y = np.where(r2[::-1] < 4, 3 - r2[::-1], 4)
    mo = c["min_overlap"]
    for d in list(range(0, l1 - mo + 1)) + list(range(-1, -(l2 - mo) - 1, -1)):
        lo, hi = max(0, -d), min(l2, l1 - d)
        ov = hi - lo
        if ov <= 0:
            continue
        xs, ys = x[lo + d:hi + d], y[lo:hi]
        diff = ov - int(np.count_nonzero((xs == ys) & (xs < 4)))
        if ov >= mo and diff <= c["max_diff"] and diff * 100 <= c["max_diff_pct"] * ov:
            return d + l2, diff
    return -1, 0


def adapter_cut(x, a, c):
    """the smallest acceptable position of the adapter (classes a) in the read (classes x), or len(x)"""
    l, m = len(x), len(a)
    for p in range(l):
        n = min(m, l - p)
        if n < c["adapter_min"]:
            break                                                             # (c only falls from here on)
        xs = x[p:p + n]
        diff = n - int(np.count_nonzero((xs == a[:n]) & (xs < 4)))
        if (diff == 0) if c["adapter_mm_per"] == 0 else (diff * c["adapter_mm_per"] <= n):
            return p
    return l


def expected(B, lens, c, codes):
    """what rfq_adapter_rows must write and report"""
    n = len(lens); pairs = c["pairs"]
    K = classes(B, codes)
    ads = [classes(np.frombuffer(a, np.uint8), False) if a else None for a in (c["adapter1"], c["adapter2"])]
    length = np.zeros(n, np.int32); how = np.zeros(n, np.uint8)
    insert = np.full(n // 2 if pairs else 0, -1, np.int32); diff = np.zeros(n // 2 if pairs else 0, np.int32)
    hist = np.zeros(c["hist_len"], np.uint64)
    s = dict.fromkeys(FIELDS, 0); s["n_rows"] = n; s["n_pairs"] = n // 2 if pairs else 0
    cut_o = [int(l) for l in lens]
    if pairs:
        assert n % 2 == 0
        for k in range(n // 2):
            l1, l2 = int(lens[2 * k]), int(lens[2 * k + 1])
            ins, df = overlap_of(K[2 * k, :l1], K[2 * k + 1, :l2], c)
            insert[k], diff[k] = ins, df
            if ins >= 0:
                s["pairs_found"] += 1
                cut_o[2 * k], cut_o[2 * k + 1] = min(l1, ins), min(l2, ins)
                if c["hist_len"]:
                    hist[min(ins, c["hist_len"] - 1)] += 1
    for i in range(n):
        l = int(lens[i])
        a = ads[i & 1] if pairs else ads[0]
        cut_a = adapter_cut(K[i, :l], a, c) if a is not None else l
        length[i] = min(cut_o[i], cut_a)
        how[i] = (BY_OVERLAP if cut_o[i] < l else 0) | (BY_ADAPTER if cut_a < l else 0)
        s["rows_cut"] += int(how[i] != 0); s["rows_cut_overlap"] += int(how[i]) & 1; s["rows_cut_adapter"] += int(how[i]) >> 1
        s["bases_in"] += l; s["bases_out"] += int(length[i])
        assert (length[i] < l) == (how[i] != 0)
    return dict(length=length, how=how, insert=insert, diff=diff, hist=hist, summary=s)


OUT_ARGS = dict(l="d_len", h="d_how", i="d_insert", d="d_diff", H="d_insert_hist")
OUT_NAMES = dict(l="length", h="how", i="insert", d="diff", H="hist")
OUT_TYPES = dict(l=np.int32, h=np.uint8, i=np.int32, d=np.int32, H=np.uint64)


def summary_of(r):
    return {f: int(getattr(r, f)) for f in FIELDS}


def outputs_for(c):
    return "lh" + ("id" if c["pairs"] else "") + ("H" if c["hist_len"] else "")


def run(codec, dev, c, codes, outputs=None):
    """one rfq_adapter_rows into Guarded buffers of exactly their size; returns (dict of numpy outputs, summary dict, raw bytes of the outputs)"""
    outputs = outputs_for(c) if outputs is None else outputs
    n = dev.n
    size = dict(l=4 * n, h=n, i=4 * (n // 2), d=4 * (n // 2), H=8 * c["hist_len"])
    g = {o: W.Guarded(codec, size[o]) for o in outputs}
    try:
        r = codec.adapter_rows(*dev.adapter_args(), codes=codes, **c, **{OUT_ARGS[o]: g[o].ptr for o in outputs})
        assert all(x.guards_intact() for x in g.values()), "a guard around an output buffer was written"
        raw = {o: x.body() for o, x in g.items()}
        return {o: np.frombuffer(raw[o], OUT_TYPES[o]) for o in outputs}, summary_of(r), raw
    finally:
        for x in g.values():
            x.free()


def compare(out, summ, e, what=""):
    for o, got in out.items():
        want = e[OUT_NAMES[o]]
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]; i = int(bad[0])
            raise AssertionError("%s %s differs in %d of %d entries, first %d: got %r, want %r" % (what, OUT_NAMES[o], len(bad), len(want), i, got[i], want[i]))
    assert summ == e["summary"], (what, {k: (summ[k], e["summary"][k]) for k in FIELDS if summ[k] != e["summary"][k]})


def check(codec, B, lens, c, codes, shifts=(0,), paths=PATHS, e=None, outputs=None, what=""):
    """the call equals the reference, at every shift and on both paths; returns the reference"""
    e = e or expected(B, lens, c, codes)
    for shift in shifts:
        dev = W.DevRows(codec, B, None, lens, shift=shift)
        try:
            for path in paths:
                codec.set_option("RFQ_ADAPTER", path)
                out, summ, _ = run(codec, dev, c, codes, outputs)
                compare(out, summ, e, "%s shift %d path %s:" % (what, shift, path or "default"))
        finally:
            codec.set_option("RFQ_ADAPTER", None)
            dev.free()
    return e


# ---------------------------------------------------------------- making reads
def enc(k, codes, rng=None):
    """classes 0 .. 3 -> base bytes: codes, or letters (in either case with an rng)"""
    k = np.asarray(k, np.uint8)
    if codes:
        return k.copy()
    up = np.frombuffer(b"ACGT", np.uint8)[k]
    return up if rng is None else np.where(rng.random(len(k)) < 0.3, up + 32, up).astype(np.uint8)


def rc(k):
    return (3 - np.asarray(k, np.uint8))[::-1]


def ad_classes(a):
    return ASCII_CLASS[np.frombuffer(a, np.uint8)]


def noise(rng, n, codes):
    """bytes of every kind: what lies behind a read"""
    return rng.integers(0, 256, n, dtype=np.uint8)


def put_row(B, i, parts):
    row = np.concatenate([np.asarray(p, np.uint8) for p in parts])[:B.shape[1]]
    B[i, :len(row)] = row


# ---------------------------------------------------------------- test 1: shapes
ROW_LENS = (1, 15, 16, 17, 63, 64, 65, 100, 150, 160, 255, 256, 257, 300, 1024, 1100)
PAIR_COUNTS = (1, 2, 127, 129)


def pair_counts(L):
    cap = 5 if L >= 1024 else (33 if L >= 255 else 129)
    return sorted({min(p, cap) for p in PAIR_COUNTS})


def random_pairs(npairs, L, seed, codes):
    """npairs pairs at stride L: lengths 0 .. L (both ends present from two pairs on); bases A C G T with N, IUPAC letters and lower case (ASCII) or codes 4, 5, 255
    here and there; a third of the pairs comes from a fragment whose insert lies below, at or above the read length, with the adapters behind it; noise behind
    every read"""
    rng = np.random.default_rng(seed)
    n = 2 * npairs
    lens = rng.integers(0, L + 1, n).astype(np.int32)
    if n >= 4:
        lens[0] = L; lens[n // 2] = 0; lens[n - 1] = L
    other = np.array([4, 5, 255], np.uint8) if codes else np.frombuffer(b"NnRYKMSWrykm.-", np.uint8)
    B = np.zeros((n, L), np.uint8)
    for i in range(n):
        row = enc(rng.integers(0, 4, L), codes, rng)
        o = rng.random(L) < 0.03
        row[o] = other[rng.integers(0, len(other), int(o.sum()))]
        B[i] = row
    a1, a2 = enc(ad_classes(AD1), codes, rng), enc(ad_classes(AD2), codes, rng)
    for k in range(npairs):
        if k % 3 != 1 and npairs > 1:
            continue
        l = int(rng.integers(max(1, L // 2), L + 1))
        ins = int(rng.choice((max(1, l // 3), max(1, l - 1), l, l + 1, l + max(1, l // 2), 2 * l + 3)))
        frag = rng.integers(0, 4, ins)
        put_row(B, 2 * k, (enc(frag, codes, rng), a1, noise(rng, L, codes)))
        put_row(B, 2 * k + 1, (enc(rc(frag), codes, rng), a2, noise(rng, L, codes)))
        lens[2 * k] = l; lens[2 * k + 1] = max(0, l - int(rng.integers(0, 3)))
    pos = np.arange(L)[None, :]
    B = np.where(pos < lens[:, None], B, rng.integers(0, 256, (n, L), dtype=np.uint8)).astype(np.uint8)
    return B, lens


def shape_criteria(L):
    mo = 4 if L < 64 else 12
    ov = dict(pairs=True, min_overlap=mo, max_diff=3, max_diff_pct=20)
    ad = dict(adapter1=AD1, adapter2=AD2, adapter_min=4, adapter_mm_per=6)
    return [("overlap", crit(**ov)), ("adapters", crit(adapter1=AD1, adapter_min=3, adapter_mm_per=5)), ("both", crit(hist_len=min(2 * L, 300) + 1, **ov, **ad))]


def check_shapes(codec, L):
    r = ROW_LENS.index(L)
    for j, npairs in enumerate(pair_counts(L)):
        codes = (j + r) % 2 == 1
        B, lens = random_pairs(npairs, L, 1000 * L + npairs, codes)
        for i, (label, c) in enumerate(shape_criteria(L)):
            e = check(codec, B, lens, c, codes, shifts=(SHIFTS[(i + j + r) % 4],), what="%s L %d pairs %d codes %d" % (label, L, npairs, codes))
            if label == "both" and npairs >= 33 and L >= 63:
                assert e["summary"]["pairs_found"] > 0 and e["summary"]["rows_cut_adapter"] > 0, e["summary"]
    B, lens = random_pairs(pair_counts(L)[-1] if L < 255 else 9, L, 7 * L, codes=r % 2 == 0)
    check(codec, B, lens, shape_criteria(L)[2][1], r % 2 == 0, shifts=SHIFTS, what="both, every shift of the buffer, L %d" % L)


# ---------------------------------------------------------------- test 2: every shift
EVERY_SHIFT = [(150, 150, 160), (64, 64, 64), (65, 65, 65), (130, 130, 144), (150, 97, 160), (97, 150, 160)]
EVERY_SHIFT_IDS = ["%d_%d" % (a, b) for a, b, _ in EVERY_SHIFT]
EVERY_CRIT = crit(pairs=True, min_overlap=20, max_diff=3, max_diff_pct=100)


def pair_at(rng, l1, l2, d, ndiff):
    """classes of (x, y): y[j] == x[j + d] on the compared positions but for exactly ndiff of them, random elsewhere"""
    x = rng.integers(0, 4, l1).astype(np.uint8); y = rng.integers(0, 4, l2).astype(np.uint8)
    lo, hi = max(0, -d), min(l2, l1 - d)
    y[lo:hi] = x[lo + d:hi + d]
    for j in rng.choice(np.arange(lo, hi), ndiff, replace=False):
        y[j] = (y[j] + 1 + rng.integers(0, 3)) % 4
    return x, y


_every_cache = {}


def every_shift_rows(label):
    """(B, lens, expected) for one length pair, made once; the host loop itself finds (d + l2, 3) for every first pair and -1 for its twin"""
    if label in _every_cache:
        return _every_cache[label]
    l1, l2, L = EVERY_SHIFT[EVERY_SHIFT_IDS.index(label)]
    rng = np.random.default_rng(20 + l1 * 7 + l2)
    ds = list(range(-(l2 - 20), l1 - 20 + 1))
    codes = l1 != 65
    B = rng.integers(0, 256, (4 * len(ds), L), dtype=np.uint8)
    for k, d in enumerate(ds):
        for t, nd in ((0, 3), (1, 4)):
            x, y = pair_at(rng, l1, l2, d, nd)
            put_row(B, 4 * k + 2 * t, (enc(x, codes, rng), B[4 * k + 2 * t, l1:]))
            put_row(B, 4 * k + 2 * t + 1, (enc(rc(y), codes, rng), B[4 * k + 2 * t + 1, l2:]))
    lens = np.tile(np.array([l1, l2], np.int32), 2 * len(ds))
    e = expected(B, lens, EVERY_CRIT, codes)
    for k, d in enumerate(ds):
        assert (e["insert"][2 * k], e["diff"][2 * k]) == (d + l2, 3), (label, d, e["insert"][2 * k], e["diff"][2 * k])
        assert (e["insert"][2 * k + 1], e["diff"][2 * k + 1]) == (-1, 0), (label, d, "twin", e["insert"][2 * k + 1])
        assert e["length"][4 * k] == min(l1, d + l2) and e["length"][4 * k + 1] == min(l2, d + l2)
    _every_cache[label] = (B, lens, e, codes)
    return _every_cache[label]


def check_every_shift(codec, label):
    B, lens, e, codes = every_shift_rows(label)
    k = EVERY_SHIFT_IDS.index(label)
    check(codec, B, lens, EVERY_CRIT, codes, shifts=(SHIFTS[k % 4], SHIFTS[(k + 1) % 4]), e=e, what="every shift " + label)


# ---------------------------------------------------------------- tests 3, 4, 5: thresholds, order, classes
def rows_of(pairs_list, L, codes, fill=None, seed=5):
    """[(r1 bytes, r2 bytes)] -> (B, lens) at stride L; behind the reads `fill` (an array generator's noise by default)"""
    rng = np.random.default_rng(seed)
    n = 2 * len(pairs_list)
    B = rng.integers(0, 256, (n, L), dtype=np.uint8) if fill is None else np.full((n, L), fill, np.uint8)
    lens = np.zeros(n, np.int32)
    for k, pr in enumerate(pairs_list):
        for t in (0, 1):
            row = np.asarray(pr[t], np.uint8)
            B[2 * k + t, :len(row)] = row; lens[2 * k + t] = len(row)
    return B, lens


def check_thresholds(codec):
    rng = np.random.default_rng(3)
    # diff * 100 == max_diff_pct * ov: 4 of 40 at 10 % is taken, 5 is not (min_overlap 40: d = 0 is the only shift with that many)
    prs = []
    for nd in (4, 5, 0):
        x, y = pair_at(rng, 40, 40, 0, nd)
        prs.append((enc(x, True), enc(rc(y), True)))
    B, lens = rows_of(prs, 48, True)
    c = crit(pairs=True, min_overlap=40, max_diff=40, max_diff_pct=10)
    e = check(codec, B, lens, c, True, shifts=(0, 7), what="pct at equality")
    assert list(e["insert"]) == [40, -1, 40] and list(e["diff"]) == [4, 0, 0]
    # ov == min_overlap is taken, min_overlap - 1 is not
    prs = []
    for d in (30, 31, -30, -31):
        x, y = pair_at(rng, 50, 50, d, 0)
        prs.append((enc(x, False, rng), enc(rc(y), False, rng)))
    B, lens = rows_of(prs, 50, False)
    e = check(codec, B, lens, crit(pairs=True, min_overlap=20, max_diff=0, max_diff_pct=0), False, shifts=(0, 1), what="ov at min_overlap")
    assert list(e["insert"]) == [80, -1, 20, -1], list(e["insert"])
    # max_diff 0: one disagreement is one too many; max_diff 2^32 - 1 with 100 %: d = 0 takes whatever it finds, its count is the full count
    prs = []
    for nd in (0, 1):
        x, y = pair_at(rng, 100, 100, 10, nd)
        prs.append((enc(x, True), enc(rc(y), True)))
    B, lens = rows_of(prs, 100, True)
    e = check(codec, B, lens, crit(pairs=True, min_overlap=30, max_diff=0, max_diff_pct=100), True, shifts=(0, 15), what="max_diff 0")
    assert list(e["insert"]) == [110, -1]
    e = check(codec, B, lens, crit(pairs=True, min_overlap=30, max_diff=0xFFFFFFFF, max_diff_pct=100), True, what="max_diff 2^32 - 1")
    assert list(e["insert"]) == [100, 100] and all(50 < v <= 100 for v in e["diff"])
    e = check(codec, B, lens, crit(pairs=True, min_overlap=0xFFFFFFFF, max_diff=0xFFFFFFFF, max_diff_pct=100), True, what="min_overlap 2^32 - 1")
    assert list(e["insert"]) == [-1, -1]


def check_order(codec):
    rng = np.random.default_rng(4)
    c = crit(pairs=True, min_overlap=20, max_diff=1, max_diff_pct=10)
    prs = []
    unit = rng.permutation(np.array([0, 1, 2, 3, 0, 2, 1], np.uint8))
    x = np.tile(unit, 14)[:96]
    prs.append((enc(x, True), enc(rc(x[14:14 + 60]), True)))                    # a tandem repeat: acceptable at d = 0, 7, 14, 21, 28, 35 and at every -7 k
    prs.append((enc(x[7:80], True), enc(rc(x), True)))                         # the same with the longer mate: d = 0 again, in front of every d < 0
    x = rng.integers(0, 4, 100).astype(np.uint8); x[70:100] = x[0:30]
    y = rng.integers(0, 4, 50).astype(np.uint8); y[0:40] = x[60:100]; y[10:50] = x[0:40]
    prs.append((enc(x, True), enc(rc(y), True)))                               # acceptable at d = 60 and at d = -10: d >= 0 comes first
    prs.append((enc(np.zeros(90, np.uint8), True), enc(rc(np.zeros(70, np.uint8)), True)))      # one base over and over: d = 0
    x = rng.integers(0, 4, 100).astype(np.uint8); y = np.concatenate([rng.integers(0, 4, 10).astype(np.uint8), x[0:40]])
    prs.append((enc(x, True), enc(rc(y), True)))                               # acceptable only at d = -10
    B, lens = rows_of(prs, 112, True)
    e = check(codec, B, lens, c, True, shifts=SHIFTS, what="order")
    assert list(e["insert"]) == [60, 96, 110, 70, 40], list(e["insert"])
    assert list(e["length"][4:10]) == [100, 50, 70, 70, 40, 40]


def check_classes(codec):
    c0 = crit(pairs=True, min_overlap=10, max_diff=0, max_diff_pct=0)
    call = crit(pairs=True, min_overlap=10, max_diff=1000, max_diff_pct=100)
    rng = np.random.default_rng(5)
    frag = rng.integers(0, 4, 40).astype(np.uint8)
    up, lo = enc(frag, False), enc(frag, False) + 32
    r2 = enc(rc(frag), False)
    prs = [(np.full(40, ord("N"), np.uint8), np.full(40, ord("N"), np.uint8)),      # N against N never agrees
           (up, r2 + 32), (lo, r2),                                                   # lower case agrees with upper case
           (np.frombuffer(b"RYKMSWBDHV" * 4, np.uint8), np.frombuffer(b"RYKMSWBDHV" * 4, np.uint8))]
    B, lens = rows_of(prs, 40, False)
    e = check(codec, B, lens, c0, False, shifts=(0, 1), what="classes, ASCII")
    assert list(e["insert"]) == [-1, 40, 40, -1]
    e = check(codec, B, lens, call, False, what="classes, ASCII, every diff")
    assert list(e["insert"]) == [40] * 4 and list(e["diff"]) == [40, 0, 0, 40]
    # an ASCII letter judged in code mode is other, a code judged in ASCII mode is other
    e = check(codec, B, lens, call, True, what="ASCII bytes as codes")
    assert list(e["diff"]) == [40] * 4
    Bc, lc = rows_of([(enc(frag, True), enc(rc(frag), True))], 40, True)
    e = check(codec, Bc, lc, call, False, what="codes as ASCII bytes")
    assert list(e["diff"]) == [40]
    e = check(codec, Bc, lc, c0, True, what="codes as codes")
    assert list(e["insert"]) == [40]
    # codes 4, 5 and 255 are other: a pair that agrees everywhere but there
    x = enc(frag, True); y = enc(rc(frag), True); x[[3, 17]] = (5, 255); y[[39 - 17, 39 - 30]] = (255, 4)
    Bo, lo_ = rows_of([(x, y)], 64, True)
    e = check(codec, Bo, lo_, call, True, shifts=(0, 7), what="codes 4, 5, 255")
    assert list(e["insert"]) == [40] and list(e["diff"]) == [3]
    # what lies behind a read continues the perfect match: the right answer does not see it
    for codes in (True, False):
        F = rng.integers(0, 4, 64).astype(np.uint8)
        r1, r2 = enc(F, codes), enc(rc(F), codes)
        for L in (64, 70):
            Bb = np.zeros((2, L), np.uint8); Bb[0, :64] = r1; Bb[1, :64] = r2
            lb = np.array([30, 30], np.int32)
            e = check(codec, Bb, lb, c0, codes, shifts=SHIFTS, what="bytes behind the reads, overlap")
            assert list(e["insert"]) == [-1] and list(e["length"]) == [30, 30]
            lb = np.array([40, 38], np.int32)                                   # x = F[0:40], y = F[26:64]: d = 26, insert 64
            e = check(codec, Bb, lb, c0, codes, shifts=(0, 15), what="bytes behind the reads, a true overlap")
            assert list(e["insert"]) == [64] and list(e["diff"]) == [0]
        ad = b"GGTTGTGTTGGT"
        row = np.concatenate([enc(rng.integers(0, 2, 30), codes), enc(ad_classes(ad), codes)])
        Ba = np.zeros((1, 48), np.uint8); Ba[0, :42] = row
        for l, want in ((30, 30), (33, 33), (34, 30), (42, 30)):
            e = check(codec, Ba, np.array([l], np.int32), crit(adapter1=ad, adapter_min=4, adapter_mm_per=0), codes, shifts=(0, 1), what="bytes behind the read, adapter")
            assert list(e["length"]) == [want], (l, e["length"])


# ---------------------------------------------------------------- test 6: the adapter at every position
ADAPTER_LENS = (1, 13, 33, 64)


def gt_adapter(m, seed):
    """an adapter of G and T only, against reads of A and C only: no chance match, so what is expected is known by construction"""
    rng = np.random.default_rng(seed)
    return bytes(np.frombuffer(b"GT", np.uint8)[rng.integers(0, 2, m)])


def check_adapter_positions(codec, m):
    rng = np.random.default_rng(60 + m)
    a1, a2 = gt_adapter(m, m), gt_adapter(m, m + 100)
    if m > 1:
        assert a1 != a2
    for l, L in ((150, 160), (65, 65)):
        for codes in (True, False):
            for amin in sorted({1, min(4, m), m}):
                # row p: the adapter at p (what falls behind the read is cut off), A / C in front and behind
                rows = []
                for p in range(l + 1):
                    body = rng.integers(0, 2, l + 64).astype(np.uint8)
                    rows.append(np.concatenate([body[:p], ad_classes(a1 if (p % 2 == 0) else a2), body[p:]])[:l])
                if len(rows) % 2:
                    rows.append(rng.integers(0, 2, l).astype(np.uint8))
                B = rng.integers(0, 256, (len(rows), L), dtype=np.uint8)
                for i, rw in enumerate(rows):
                    B[i, :l] = enc(rw, codes, rng)
                lens = np.full(len(rows), l, np.int32)
                # with pairs: even rows adapter 1, odd rows adapter 2 - rows p are made that way
                c = crit(pairs=True, min_overlap=L + 1, adapter1=a1, adapter2=a2, adapter_min=amin, adapter_mm_per=0)
                e = check(codec, B, lens, c, codes, shifts=(SHIFTS[(m + amin) % 4],), what="adapter %d at every p, pairs, amin %d" % (m, amin))
                for p in range(l + 1):
                    assert e["length"][p] == (p if l - p >= amin else l), (m, l, amin, p, e["length"][p])
                # without pairs every row uses adapter 1: the odd rows hold adapter 2
                if m >= 13 and amin == 4:
                    c1 = crit(adapter1=a1, adapter_min=amin, adapter_mm_per=0)
                    e = check(codec, B, lens, c1, codes, shifts=(SHIFTS[m % 4],), what="adapter %d at every p, no pairs" % m)
                    assert all(e["length"][p] == (p if l - p >= amin else l) for p in range(0, l + 1, 2))
                    odd = [p for p in range(1, l + 1 - m, 2)]                   # (adapter 2 whole inside the read: adapter 1 does not cut there but by chance)
                    assert len(odd) < 8 or sum(1 for p in odd if e["length"][p] == p) < len(odd) // 4
                    # one adapter off
                    e = check(codec, B, lens, crit(pairs=True, min_overlap=L + 1, adapter2=a2, adapter_min=amin, adapter_mm_per=0), codes, what="adapter 1 off")
                    assert all(e["length"][p] == l for p in range(0, l + 1, 2)) and e["length"][1] == 1
    # diff_a * adapter_mm_per == c is found, one more is not; the earliest of two matches wins
    for m2, per, nd in ((64, 8, 8), (33, 11, 3), (13, 13, 1), (13, 4, 3)):
        a = gt_adapter(m2, 7 * m2 + per)
        k = ad_classes(a)
        rows = []
        for extra in (0, 1):
            for p in (0, 1, 17, 63, 64, 86):
                body = rng.integers(0, 2, 150).astype(np.uint8)
                bad = k.copy()
                for j in rng.choice(m2, nd + extra, replace=False):
                    bad[j] = bad[j] - 2                                         # G -> A, T -> C
                rows.append(np.concatenate([body[:p], bad, body[p + m2:]])[:150])
        body = rng.integers(0, 2, 150).astype(np.uint8)
        rows.append(np.concatenate([body[:20], k, body[:9], k, body])[:150])   # two matches: the earliest wins
        B = rng.integers(0, 256, (len(rows), 150), dtype=np.uint8)
        for i, rw in enumerate(rows):
            B[i] = enc(rw, True)
        lens = np.full(len(rows), 150, np.int32)
        e = check(codec, B, lens, crit(adapter1=a, adapter_min=m2, adapter_mm_per=per), True, shifts=(0, 7), what="adapter mismatches at equality")
        assert list(e["length"][:12]) == [0, 1, 17, 63, 64, 86] + [150] * 6, (m2, per, list(e["length"]))
        # (a quarter of 13 bases may differ in the last set: a shifted copy of the adapter may pass, in front of the first match)
        assert e["length"][12] == 20 if per > 4 else 7 < e["length"][12] <= 20, (m2, per, e["length"][12])


# ---------------------------------------------------------------- test 7: both detectors
def check_both(codec):
    rng = np.random.default_rng(7)
    L = 160
    a1, a2 = enc(ad_classes(AD1), False), enc(ad_classes(AD2), False)
    prs = []
    for rep in range(6):
        f = rng.integers(0, 4, 90 + rep)
        prs.append((np.concatenate([enc(f, False, rng), noise(rng, 60, False)])[:150], np.concatenate([enc(rc(f), False, rng), noise(rng, 60, False)])[:150]))   # how 1 1
        x = rng.integers(0, 4, 150); y = rng.integers(0, 4, 150)
        prs.append((np.concatenate([enc(x[:100 + rep], False), a1, enc(x, False)])[:150], enc(y, False)))                                             # how 2 0
        prs.append((np.concatenate([enc(f, False, rng), a1, noise(rng, 60, False)])[:150], np.concatenate([enc(rc(f), False, rng), a2, noise(rng, 60, False)])[:150]))   # how 3 3
        prs.append((enc(x, False), enc(y, False)))                                                                                                   # how 0 0
        g = rng.integers(0, 4, 120)
        prs.append((np.concatenate([enc(g[:50], False), a1, enc(g[63:], False), noise(rng, 40, False)])[:150], np.concatenate([enc(rc(g), False), noise(rng, 40, False)])[:150]))
    B, lens = rows_of(prs, L, False)
    c = crit(pairs=True, min_overlap=30, max_diff=20, max_diff_pct=20, adapter1=AD1, adapter2=AD2, adapter_min=4, adapter_mm_per=8, hist_len=200)
    e = check(codec, B, lens, c, False, shifts=(0, 1, 7, 15), what="both detectors")
    assert [list(e["how"][2 * k:2 * k + 2]) for k in range(5)] == [[1, 1], [2, 0], [3, 3], [0, 0], [3, 1]], list(e["how"][:10])
    assert e["length"][8] == 50 and e["insert"][4] == 120 and e["length"][9] == 120            # len is the smaller of the two cuts
    s = e["summary"]
    assert s["n_pairs"] == 30 and s["pairs_found"] == 18 and s["rows_cut_overlap"] == 36 and s["rows_cut_adapter"] == 24 and s["rows_cut"] == 42, s
    assert s["bases_in"] == 150 * 60 and s["bases_out"] == int(e["length"].sum())


# ---------------------------------------------------------------- test 8: degenerate
def check_degenerate(codec):
    both = crit(pairs=True, min_overlap=12, max_diff=3, max_diff_pct=20, adapter1=AD1, adapter2=AD2, adapter_min=4, adapter_mm_per=6, hist_len=64)
    for L in (16, 40, 300):
        B, lens = random_pairs(35, L, 80 + L, codes=True)
        zero = np.zeros_like(lens)
        e = check(codec, B, zero, both, True, shifts=(0, 15), what="all lengths 0")
        assert e["summary"]["bases_in"] == 0 and e["summary"]["pairs_found"] == 0 and not e["hist"].any()
        e = check(codec, B, np.minimum(lens, 11), both, True, shifts=(0, 1), what="lengths below min_overlap")
        assert e["summary"]["pairs_found"] == 0
        e = check(codec, B, lens, crit(), True, shifts=(0, 7), what="neither detector")
        assert np.array_equal(e["length"], lens) and not e["how"].any() and e["summary"]["rows_cut"] == 0
        e = check(codec, B, lens, crit(pairs=True, min_overlap=L + 1, max_diff=L, max_diff_pct=100), True, what="min_overlap above row_len")
        assert e["summary"]["pairs_found"] == 0 and list(e["insert"]) == [-1] * 35
        check(codec, B[:1], lens[:1], crit(adapter1=AD1, adapter_min=1, adapter_mm_per=2), True, what="one row")
    g = W.Guarded(codec, 8 * 5)
    try:
        r = codec.adapter_rows(0, 0, None, None, hist_len=5, d_insert_hist=g.ptr, **{k: v for k, v in both.items() if k != "hist_len"})
        assert summary_of(r) == dict.fromkeys(FIELDS, 0) and g.guards_intact() and g.body() == b"\0" * 40
        assert summary_of(codec.adapter_rows(0, 160, None, None)) == dict.fromkeys(FIELDS, 0)
    finally:
        g.free()


# ---------------------------------------------------------------- test 9: outputs
def check_outputs(codec):
    B, lens = random_pairs(120, 150, 9, codes=False)
    c = crit(pairs=True, min_overlap=15, max_diff=3, max_diff_pct=20, adapter1=AD1, adapter2=AD2, adapter_min=4, adapter_mm_per=6, hist_len=151)
    e = expected(B, lens, c, False)
    assert 10 < e["summary"]["pairs_found"] < 120 and all(e["summary"][f] > 0 for f in FIELDS), e["summary"]
    eh_by = {hl: expected(B, lens, dict(c, hist_len=hl), False) for hl in (1, 2, 151, 400, 65536)}
    dev = W.DevRows(codec, B, None, lens, shift=3)
    try:
        for path in PATHS:
            codec.set_option("RFQ_ADAPTER", path)
            for outputs in ("l", "h", "i", "d", "H", "", "lhidH"):
                out, summ, raw = run(codec, dev, c, False, outputs)
                compare(out, summ, e, "outputs %r" % outputs)
            out2, summ2, raw2 = run(codec, dev, c, False, "lhidH")
            assert raw2 == raw and summ2 == summ, "the same call on the same context gave other bytes"
            for hl in (1, 2, 151, 400, 65536):
                eh = eh_by[hl]
                out, summ, _ = run(codec, dev, dict(c, hist_len=hl), False, "H")
                compare(out, summ, eh, "hist_len %d" % hl)
                assert int(eh["hist"].sum()) == eh["summary"]["pairs_found"] < eh["summary"]["n_pairs"]
                if hl <= 2:
                    assert eh["hist"][hl - 1] > 0                                 # (the clamp bin)
    finally:
        codec.set_option("RFQ_ADAPTER", None)
        dev.free()


# ---------------------------------------------------------------- test 10: refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, lens = random_pairs(20, 33, 9, codes=True)
    check(codec, B, lens, shape_criteria(33)[2][1], True, paths=(None,), what="after a refusal")


def check_host_refusals(codec):
    import _rows_enc as R
    from repaq_amd import RfqError
    n, L = 40, 32
    B, lens = random_pairs(n // 2, L, 10, codes=False)
    dev = W.DevRows(codec, B, None, lens)
    buf = codec.dev_put(b"\0" * 8192); b = buf.value
    try:
        rows = dev.adapter_args()

        def at(p, k):
            return C.c_void_p(p.value + k)
        J = codec.adapter_rows
        ov = dict(pairs=True, min_overlap=10, max_diff=2, max_diff_pct=10)
        ad = dict(adapter1=AD1, adapter_min=4, adapter_mm_per=8)
        calls = (("odd n_rows with pairs", lambda: J(n - 1, L, dev.bases, dev.lens, **ov)),
                 ("min_overlap 0", lambda: J(*rows, **dict(ov, min_overlap=0))),
                 ("max_diff_pct 101", lambda: J(*rows, **dict(ov, max_diff_pct=101))),
                 ("adapter of 65", lambda: J(*rows, **dict(ad, adapter1=b"ACGT" * 16 + b"A"))),
                 ("adapter with N", lambda: J(*rows, **dict(ad, adapter1=b"ACGNT"))),
                 ("adapter 2 with a code", lambda: J(*rows, **ov, **ad, adapter2=b"ACG\x00")),
                 ("adapter 2 without pairs", lambda: J(*rows, **ad, adapter2=AD2)),
                 ("d_insert without pairs", lambda: J(*rows, **ad, d_insert=C.c_void_p(b))),
                 ("d_diff without pairs", lambda: J(*rows, **ad, d_diff=C.c_void_p(b))),
                 ("d_insert_hist without pairs", lambda: J(*rows, **ad, hist_len=4, d_insert_hist=C.c_void_p(b))),
                 ("adapter_min 0", lambda: J(*rows, **dict(ad, adapter_min=0))),
                 ("adapter_min 65", lambda: J(*rows, **dict(ad, adapter_min=65))),
                 ("hist_len 0 with a histogram", lambda: J(*rows, **ov, hist_len=0, d_insert_hist=C.c_void_p(b))),
                 ("hist_len 65537", lambda: J(*rows, **ov, hist_len=65537)),
                 ("no bases", lambda: J(n, L, None, dev.lens, **ov)),
                 ("row_len 0", lambda: J(n, 0, dev.bases, dev.lens, **ov)),
                 ("bad base_mode", lambda: J(*rows, **ov, base_mode=2)),
                 ("misaligned d_lens", lambda: J(n, L, dev.bases, at(dev.lens, 2), **ov)),
                 ("misaligned d_len", lambda: J(*rows, **ov, d_len=C.c_void_p(b + 2))),
                 ("misaligned d_insert", lambda: J(*rows, **ov, d_insert=C.c_void_p(b + 1))),
                 ("misaligned d_diff", lambda: J(*rows, **ov, d_diff=C.c_void_p(b + 3))),
                 ("misaligned d_insert_hist", lambda: J(*rows, **ov, hist_len=4, d_insert_hist=C.c_void_p(b + 4))),
                 ("len on lens", lambda: J(*rows, **ov, d_len=dev.lens)),
                 ("how on the last base", lambda: J(*rows, **ov, d_how=at(dev.bases, n * L - 1))),
                 ("insert ends in bases", lambda: J(*rows, **ov, d_insert=C.c_void_p(((dev.bases.value - 4 * (n // 2) + 4) & ~3)))),
                 ("diff on the last length", lambda: J(*rows, **ov, d_diff=at(dev.lens, 4 * (n - 1)))),
                 ("hist on bases", lambda: J(*rows, **ov, hist_len=2, d_insert_hist=C.c_void_p((dev.bases.value + 15) & ~7))))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3, (what, ei.value)
            _good(codec)
        # (neither detector is no error, a hist_len without a histogram is not looked at, outputs that lie on nothing are taken)
        assert J(*rows).rows_cut == 0
        assert J(*rows, **ov, hist_len=9, d_len=C.c_void_p(b), d_insert=C.c_void_p(b + 1024), d_insert_hist=C.c_void_p(b + 4096)).n_pairs == n // 2
    finally:
        dev.free(); codec.dev_free(buf)


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "middle", "last")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    import _rows_enc as R
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    for L, npairs in ((24, 150), (300, 5), (1100, 3)):
        n = 2 * npairs
        B, lens = random_pairs(npairs, L, 11, codes=True)
        row = dict(first=0, middle=n // 2 + 1, last=n - 1)[where]
        lens[row] = -1 if value == "negative" else L + 1
        lens[row ^ 1] = L                                                   # (a good row beside it)
        dev = W.DevRows(codec, B, None, lens, shift=1)
        c = shape_criteria(L)[2][1]
        try:
            for path in PATHS:
                codec.set_option("RFQ_ADAPTER", path)
                for outputs in ("", None):
                    with R.pytest_raises(RfqError) as ei:
                        run(codec, dev, c, True, outputs)
                    assert ei.value.code == -3 and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                codec.set_option("RFQ_ADAPTER", None)
                _good(codec)
        finally:
            codec.set_option("RFQ_ADAPTER", None)
            dev.free()


# ---------------------------------------------------------------- test 11: adapter -> judge -> select
COMPOSE_A = crit(pairs=True, min_overlap=20, max_diff=3, max_diff_pct=10, adapter1=AD1, adapter2=AD2, adapter_min=4, adapter_mm_per=8)


def compose_text(pairs=300, seed=12):
    """two FASTQ texts of `pairs` records of 150 bases from fragments of 40 .. 400 bases with the adapters behind them; scores that fall off towards the end"""
    rng = np.random.default_rng(seed)
    out = [[], []]
    a = (AD1 + b"ACGTTGCATTGACCA" * 12, AD2 + b"TTGACGGATCAGGCA" * 12)
    for k in range(pairs):
        ins = int(rng.integers(40, 401))
        f = rng.integers(0, 4, ins)
        for m, fr in ((0, f), (1, rc(f))):
            s = (bytes(enc(fr, False)) + a[m])[:150]
            q = np.clip(38 - np.arange(150) * int(rng.integers(0, 30)) // 150 + rng.integers(-4, 5, 150), 2, 41).astype(np.uint8)
            out[m].append(b"@frag.%d %d/%d\n" % (k + 1, ins, m + 1) + s + b"\n+\n" + bytes(q + 33) + b"\n")
    return out


def compose_expected(recs, ca, cj, min_len):
    """the two texts adapter removal, the judge on the shortened reads and the pair rule leave"""
    import _judge as J
    rows = [rec.split(b"\n")[:4] for rec in recs]
    L = max(len(r[1]) for r in rows)
    B = np.zeros((len(rows), L), np.uint8); lens = np.array([len(r[1]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        B[i, :len(r[1])] = np.frombuffer(r[1], np.uint8)
    e = expected(B, lens, ca, False)
    verdicts = []
    for i, (name, s, _, q) in enumerate(rows):
        l = int(e["length"][i])
        k, a, m, _, _ = J.judge_row(list(s), [x - 33 for x in q], l, cj, False)
        verdicts.append((k and m >= min_len, name, s[a:a + m], q[a:a + m]))
    out = [[], []]
    for i in range(0, len(verdicts), 2):
        if verdicts[i][0] and verdicts[i + 1][0]:
            for m in (0, 1):
                _, name, s, q = verdicts[i + m]
                out[m].append(name + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out[0]), b"".join(out[1]), len(out[0]), e


def check_composition(codec):
    import _judge as J
    import _select as S
    from repaq_amd import PE_TWO_FILES
    t1, t2 = compose_text()
    fq1, fq2 = b"".join(t1), b"".join(t2)
    cj = J.crit(cut_flags=J.TAIL, cut_window=4, cut_mean_q=20, min_len=80, min_mean_q=20)
    w1, w2, kept, e = compose_expected([x for pair in zip(t1, t2) for x in pair], COMPOSE_A, cj, 80)
    assert 100 < kept < 290 and e["summary"]["rows_cut"] > 100, (kept, e["summary"])
    _, B, Q, lens, names = codec.text_rows_bytes(fq1, fq2, paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    dev = W.DevRows(codec, B, Q, lens, names)
    ga, gk, gs, gl = W.Guarded(codec, 4 * n), W.Guarded(codec, n), W.Guarded(codec, 4 * n), W.Guarded(codec, 4 * n)
    bufs = []
    try:
        a = codec.adapter_rows(n, 160, dev.bases, dev.lens, d_len=ga.ptr, **COMPOSE_A)
        assert summary_of(a) == e["summary"] and ga.guards_intact()
        j = codec.judge_rows(n, 160, dev.bases, dev.quals, ga.ptr, **cj, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
        assert j.n_rows == n and all(g.guards_intact() for g in (gk, gs, gl))
        sel = dict(d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr, pairs=True, min_len=80)
        q = codec.select_rows(*dev.args(), **sel)
        m, L, nl = int(q.n_rows), max(int(q.max_len), 1), int(q.names_len)
        assert m == 2 * kept
        ob, oq, ol, on, oo = (codec.dev_put(b"\0" * max(k, 1)) for k in (m * L, m * L, 4 * m, nl, 8 * (m + 1)))
        bufs += [ob, oq, ol, on, oo]
        codec.select_rows(*dev.args(), row_len=L, out_bases=ob, bases_cap=m * L, out_quals=oq, quals_cap=m * L, out_lens=ol, lens_cap=m, out_names=on,
                          names_cap=nl, out_name_off=oo, off_cap=m + 1, **sel)
        r = codec.rows_to_text(m, L, ob, oq, ol, on, nl, oo, paired=PE_TWO_FILES, qual_offset=33)
        got = (codec.dev_get(r.d_fq1, r.n1), codec.dev_get(r.d_fq2, r.n2))
        assert got == (w1, w2), "the texts differ from the host's"
    finally:
        dev.free()
        for g in (ga, gk, gs, gl):
            g.free()
        for p in bufs:
            codec.dev_free(p)


# ---------------------------------------------------------------- test 12: the seams of the shared walk
AR_ITER = 4                                                                   # (enc/rows_adapter.h)
_walk_sets = {}


def walk_sets(L, counts):
    """per count of PAIRS: rows, mode and the reference under overlap and adapters at once - made once per row length, shared by the default and the general path"""
    if L not in _walk_sets:
        c = shape_criteria(L)[2][1]
        _walk_sets[L] = [(random_pairs(p, L, 31 * L + p, p % 2 == 1), p % 2 == 1) for p in counts]
        _walk_sets[L] = [(B, lens, codes, expected(B, lens, c, codes)) for (B, lens), codes in _walk_sets[L]]
    return _walk_sets[L]


def check_walk(codec, label):
    L, path, counts = W.walk_case(label, AR_ITER)
    for B, lens, codes, e in walk_sets(L, counts):
        check(codec, B, lens, shape_criteria(L)[2][1], codes, shifts=(len(lens) % 16,), paths=(path,), e=e, what="walk L %d pairs %d" % (L, len(lens) // 2))


def check_walk_bad_length(codec):
    """a bad length in R2 of the last pair, a workgroup's first pair behind its last step: the refusal names the row"""
    import _rows_enc as R
    from repaq_amd import RfqError
    for L in (256, 272):
        n = 2 * (256 // (16 if L <= 256 else 64) * AR_ITER + 1)
        B, lens = random_pairs(n // 2, L, 5, codes=True)
        lens[n - 1] = L + 1
        dev = W.DevRows(codec, B, None, lens)
        try:
            with R.pytest_raises(RfqError) as ei:
                run(codec, dev, shape_criteria(L)[2][1], True)
            assert ei.value.code == -3 and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
        finally:
            dev.free()
