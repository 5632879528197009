"""Shared helpers of the rfq_judge_rows tests (tests/test_emu_judge.py on the SIMT interpreter, tests/test_gpu_judge.py on the MI355X).

Nothing expected comes from the code under test: judge_row() is a plain loop over one row written from the rules in include/rfq_hip.h (prefix sums of the
row's scores, nothing else, help it along), expected() calls it per row and adds up the summary.  Every output goes into a _rows.Guarded buffer of exactly
n_rows entries, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R

FRONT, RIGHT, TAIL = 1, 2, 4
SHORT, MANY_N, MEANQ, LOWQ, COMPLEX = 1, 2, 4, 8, 16
DEFAULTS = dict(trim_front=0, trim_tail=0, poly_g=0, cut_flags=0, cut_window=0, cut_mean_q=0, max_len=0, min_len=0, max_n=-1, min_mean_q=0, qual_q=0,
                max_lowq_pct=0, min_complexity_pct=0)
FIELDS = ("n_rows", "n_kept", "why_short", "why_n", "why_meanq", "why_lowq", "why_complex", "bases_in", "qsum_in", "q20_in", "q30_in", "bases_out", "qsum_out",
          "q20_out", "q30_out")


def crit(**kw):
    c = dict(DEFAULTS); c.update(kw)
    assert set(c) == set(DEFAULTS), sorted(set(c) - set(DEFAULTS))
    return c


def judge_row(b, q, l, c, codes):
    """(keep, start, len, why, (qsum, n_cnt, lowq, trans)) of one row: b, q its bytes as lists of ints, l its length"""
    G, N = ((2,), (4,)) if codes else ((71, 103), (78, 110))
    P = [0] * (l + 1)
    for i in range(l):
        P[i + 1] = P[i] + q[i]
    a = min(c["trim_front"], l); e = max(a, l - min(c["trim_tail"], l))
    if c["poly_g"] > 0 and e > a:
        r = 0
        while e - 1 - r >= a and b[e - 1 - r] in G:
            r += 1
        if r >= c["poly_g"]:
            e -= r
    cw, mq = c["cut_window"], c["cut_mean_q"]
    if c["cut_flags"] & FRONT and e > a:
        w = min(cw, e - a)
        for p in range(a, e - w + 1):
            if P[p + w] - P[p] >= mq * w:
                a = p
                break
        else:
            e = a
    if c["cut_flags"] & RIGHT and e > a:
        w = min(cw, e - a)
        for p in range(a, e - w + 1):
            if P[p + w] - P[p] < mq * w:
                e = p
                break
    if c["cut_flags"] & TAIL and e > a:
        w = min(cw, e - a)
        for p in range(e - w, a - 1, -1):
            if P[p + w] - P[p] >= mq * w:
                e = p + w
                break
        else:
            e = a
    if c["max_len"] > 0:
        e = min(e, a + c["max_len"])
    n = e - a
    qsum = P[e] - P[a]
    n_cnt = sum(1 for j in range(a, e) if b[j] in N)
    lowq = sum(1 for j in range(a, e) if q[j] < c["qual_q"]) if c["qual_q"] else 0
    trans = sum(1 for j in range(a, e - 1) if b[j] != b[j + 1])
    why = 0
    if n < c["min_len"]:
        why |= SHORT
    if c["max_n"] >= 0 and n_cnt > c["max_n"]:
        why |= MANY_N
    if qsum < c["min_mean_q"] * n:
        why |= MEANQ
    if c["qual_q"] > 0 and lowq * 100 > c["max_lowq_pct"] * n:
        why |= LOWQ
    if n > 1 and trans * 100 < c["min_complexity_pct"] * (n - 1):
        why |= COMPLEX
    return (1 if why == 0 else 0), a, n, why, (qsum, n_cnt, lowq, trans)


def expected(B, Q, lens, c, codes):
    """what rfq_judge_rows must write and report: keep, start, len, why, metrics as numpy arrays and the summary as a dict"""
    n = len(lens)
    keep = np.zeros(n, np.uint8); start = np.zeros(n, np.int32); length = np.zeros(n, np.int32); why = np.zeros(n, np.uint8); met = np.zeros((n, 4), np.uint32)
    s = dict.fromkeys(FIELDS, 0); s["n_rows"] = n
    Bl, Ql = B.tolist(), Q.tolist()
    for i in range(n):
        l = int(lens[i]); b, q = Bl[i], Ql[i]
        k, a, m, y, mt = judge_row(b, q, l, c, codes)
        keep[i], start[i], length[i], why[i], met[i] = k, a, m, y, mt
        s["n_kept"] += k
        for bit, f in ((SHORT, "why_short"), (MANY_N, "why_n"), (MEANQ, "why_meanq"), (LOWQ, "why_lowq"), (COMPLEX, "why_complex")):
            s[f] += 1 if y & bit else 0
        s["bases_in"] += l; s["qsum_in"] += sum(q[:l]); s["q20_in"] += sum(1 for x in q[:l] if x >= 20); s["q30_in"] += sum(1 for x in q[:l] if x >= 30)
        if k:
            w = q[a:a + m]
            s["bases_out"] += m; s["qsum_out"] += mt[0]; s["q20_out"] += sum(1 for x in w if x >= 20); s["q30_out"] += sum(1 for x in w if x >= 30)
    assert s["n_kept"] + int((why != 0).sum()) == n
    return dict(keep=keep, start=start, length=length, why=why, metrics=met, summary=s)


OUT_SIZES = dict(k=1, s=4, l=4, w=1, m=16)
OUT_ARGS = dict(k="d_keep", s="d_start", l="d_len", w="d_why", m="d_metrics")


def summary_of(r):
    return {f: int(getattr(r, f)) for f in FIELDS}


def run(codec, dev, c, codes, outputs="kslwm"):
    """one rfq_judge_rows into Guarded buffers of exactly n_rows entries; returns (dict of numpy outputs, summary dict, raw bytes of the outputs)"""
    n = dev.n
    g = {o: W.Guarded(codec, OUT_SIZES[o] * n) for o in outputs}
    try:
        r = codec.judge_rows(*dev.judge_args(), codes=codes, **c, **{OUT_ARGS[o]: g[o].ptr for o in outputs})
        assert all(x.guards_intact() for x in g.values()), "a guard around an output buffer was written"
        raw = {o: x.body() for o, x in g.items()}
        dt = dict(k=np.uint8, s=np.int32, l=np.int32, w=np.uint8, m=np.uint32)
        out = {o: np.frombuffer(raw[o], dt[o]) for o in outputs}
        if "m" in out:
            out["m"] = out["m"].reshape(n, 4)
        return out, summary_of(r), raw
    finally:
        for x in g.values():
            x.free()


def compare(out, summ, e, what=""):
    names = dict(k="keep", s="start", l="length", w="why", m="metrics")
    for o, got in out.items():
        want = e[names[o]]
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
            i = int(bad[0])
            raise AssertionError("%s %s differs in %d of %d rows, first row %d: got %r, want %r (start %d len %d why %d / start %d len %d why %d)" % (
                what, names[o], len(bad), len(want), i, got[i], want[i], out.get("s", e["start"])[i], out.get("l", e["length"])[i], out.get("w", e["why"])[i],
                e["start"][i], e["length"][i], e["why"][i]))
    assert summ == e["summary"], (what, {k: (summ[k], e["summary"][k]) for k in FIELDS if summ[k] != e["summary"][k]})
    assert summ["n_kept"] + int((e["why"] != 0).sum()) == summ["n_rows"]


def check(codec, B, Q, lens, c, codes, shifts=(0,), paths=(None, "general"), e=None, outputs="kslwm", what=""):
    """the call equals the reference, at every shift and on both paths; returns the reference"""
    e = e or expected(B, Q, lens, c, codes)
    for shift in shifts:
        dev = W.DevRows(codec, B, Q, lens, shift=shift)
        try:
            for path in paths:
                codec.set_option("RFQ_JUDGE", path)
                out, summ, _ = run(codec, dev, c, codes, outputs)
                compare(out, summ, e, "%s shift %d path %s:" % (what, shift, path or "default"))
        finally:
            codec.set_option("RFQ_JUDGE", None)
            dev.free()
    return e


# ---------------------------------------------------------------- test 1: every step alone, then all together
ROW_LENS = (1, 15, 16, 17, 100, 150, 160, 255, 256, 257, 300)
N_ROWS = (1, 2, 255, 257, 2049)
SHIFTS = (0, 1, 7, 15)
FILTERS = dict(min_len=20, max_n=2, min_mean_q=22, qual_q=15, max_lowq_pct=30, min_complexity_pct=40)
STEPS = [("trim", crit(trim_front=3, trim_tail=5)), ("poly_g", crit(poly_g=4)), ("front", crit(cut_flags=FRONT, cut_window=4, cut_mean_q=20)),
         ("right", crit(cut_flags=RIGHT, cut_window=4, cut_mean_q=20)), ("tail", crit(cut_flags=TAIL, cut_window=5, cut_mean_q=18)), ("max_len", crit(max_len=37)),
         ("filters", crit(**FILTERS)),
         ("all", crit(trim_front=2, trim_tail=1, poly_g=5, cut_flags=FRONT | RIGHT | TAIL, cut_window=4, cut_mean_q=17, max_len=140, **FILTERS))]


def random_rows(n, L, seed, codes):
    """n rows of stride L: lengths 0 .. L (both ends present from three rows on), bases ACGTN (either case in ASCII mode) with G tails and N runs here and there,
    scores that are good in the middle of a read and fall off towards its ends, a few bytes of 255; what lies behind a read is noise"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, L + 1, n).astype(np.int32)
    if n >= 3:
        lens[0] = L; lens[n // 2] = 0; lens[n - 1] = L
    alpha = np.array([0, 1, 2, 3, 4], np.uint8) if codes else np.frombuffer(b"ACGTNacgtn", np.uint8)
    p = np.array([.24, .24, .24, .24, .04]) if codes else np.array([.2, .2, .2, .2, .03, .04, .04, .04, .03, .01])
    B = alpha[rng.choice(len(alpha), (n, L), p=p / p.sum())]
    pos = np.arange(L)[None, :]
    tail = rng.integers(0, 9, n)[:, None] * (rng.random(n) < 0.4)[:, None]           # a run of G at the end of four reads in ten
    gch = np.uint8(2) if codes else np.where(rng.random((n, L)) < 0.8, np.uint8(71), np.uint8(103))
    B = np.where((pos >= lens[:, None] - tail) & (pos < lens[:, None]), gch, B).astype(np.uint8)
    mono = (rng.random(n) < 0.1)[:, None]                                              # one read in ten is one base over and over
    B = np.where(mono & (pos < lens[:, None]), B[:, :1], B).astype(np.uint8)
    edge = np.minimum(pos, np.maximum(lens[:, None] - 1 - pos, 0))
    ramp = rng.integers(1, 8, n)[:, None]
    Q = np.clip(8 + edge * 30 // (ramp * 4) + rng.integers(-9, 10, (n, L)), 0, 41)
    Q = np.where(rng.random((n, L)) < 0.01, 255, Q).astype(np.uint8)
    noise = rng.integers(0, 256, (n, L), dtype=np.uint8)
    inside = pos < lens[:, None]
    return np.where(inside, B, noise).astype(np.uint8), np.where(inside, Q, noise).astype(np.uint8), lens


def check_steps(codec, L):
    r = ROW_LENS.index(L)
    sets = [(random_rows(n, L, 1000 * L + n, codes=(j + r) % 2 == 1), (j + r) % 2 == 1) for j, n in enumerate(N_ROWS)]
    for i, (label, c) in enumerate(STEPS):
        for j in (range(len(sets)) if label == "all" else ((i + r) % 4, (i + r + 2) % 4)):
            (B, Q, lens), codes = sets[j]
            check(codec, B, Q, lens, c, codes, shifts=(SHIFTS[(i + j) % 4],), what="%s n %d codes %d" % (label, len(lens), codes))
    (B, Q, lens), codes = sets[3]
    check(codec, B, Q, lens, STEPS[-1][1], codes, shifts=SHIFTS, what="all, every shift")


# ---------------------------------------------------------------- test 2: window seams
def seam_rows(L, w, kind, positions, mq=20):
    """for every p two rows of L scores: the window of w at p is the first good one (front) / the first bad one (right) / the last good one (tail) with a sum
    of exactly mq * w (good) or of one less (bad), and in a second row that window is on the other side of the threshold by one: no such window anywhere"""
    rows = []
    for p in positions:
        assert 0 <= p <= L - w
        q = np.zeros(L, np.int64) if kind in ("front", "tail") else np.full(L, mq, np.int64)
        if kind in ("front", "tail"):
            q[p:p + w] = mq
            other = q.copy(); other[p + (w - 1 if kind == "front" else 0)] = mq - 1
        else:
            other = q.copy()
            q[p + w - 1] = mq - 1
        rows += [q, other]
    return np.array(rows).astype(np.uint8)


def check_seams(codec, kind, w, L=300, step=1, trim=0, paths=(None, "general")):
    flag = dict(front=FRONT, right=RIGHT, tail=TAIL)[kind]
    wl = min(w, L - 2 * trim)
    Q = seam_rows(L, wl, kind, range(trim, L - trim - wl + 1, step))
    n = len(Q)
    pad = (-L) % 16 + (16 if kind == "tail" else 0)                          # (the stride: whole groups, and not)
    Q = np.concatenate([Q, np.full((n, pad), 40, np.uint8)], axis=1)
    B = np.random.default_rng(w).integers(0, 4, Q.shape).astype(np.uint8)
    lens = np.full(n, L, np.int32)
    c = crit(cut_flags=flag, cut_window=w, cut_mean_q=20, trim_front=trim, trim_tail=trim)
    e = check(codec, B, Q, lens, c, True, shifts=(0, 7) if step == 1 else (3,), paths=paths, what="%s w %d" % (kind, w))
    # the reference itself finds what the rows were made for
    ps = list(range(trim, L - trim - wl + 1, step))
    for k, p in enumerate(ps):
        a, m = int(e["start"][2 * k]), int(e["length"][2 * k]); a2, m2 = int(e["start"][2 * k + 1]), int(e["length"][2 * k + 1])
        if kind == "front":
            assert (a, m) == (p, L - trim - p) and (a2, m2) == (trim, 0), (kind, p, a, m, a2, m2)
        elif kind == "right":
            assert (a, m) == (trim, p - trim) and (a2, m2) == (trim, L - 2 * trim), (kind, p, a, m, a2, m2)
        else:
            assert (a, m) == (trim, p + wl - trim) and (a2, m2) == (trim, 0), (kind, p, a, m, a2, m2)


# ---------------------------------------------------------------- test 3: poly-G
def check_poly_g(codec):
    L, pg = 48, 6
    rows = []

    def row(seq, l=None):
        rows.append((seq.ljust(L, b"G")[:L], len(seq) if l is None else l))   # (what lies behind a read is G too: it must not count)
    body = b"ACTACTACTACTACTACTACTACTAC"
    row(body + b"G" * (pg - 1)); row(body + b"G" * pg); row(body + b"G" * (pg + 9))
    row(body + b"GGG" + b"A" + b"GGG"); row(body + b"G" * pg + b"T" + b"G" * (pg - 1)); row(body + b"GGGGGGA")
    row(b"G" * 30); row(b"G" * L); row(b"G" * (pg - 1)); row(b"G" * pg); row(b"")
    row(body + b"GGgGgg"); row(body + b"ggggg"); row(body + b"gggggggg")
    row(b"GGGGGGGG" + body)
    B = np.array([np.frombuffer(s, np.uint8) for s, _ in rows]); lens = np.array([l for _, l in rows], np.int32)
    Q = np.full(B.shape, 30, np.uint8)
    code = np.where(np.isin(B, (71, 103)), 2, np.where(B == 65, 0, np.where(B == 67, 1, 3))).astype(np.uint8)
    for c in (crit(poly_g=pg), crit(poly_g=pg, trim_tail=2), crit(poly_g=pg, trim_tail=pg + 2, trim_front=3), crit(poly_g=1), crit(poly_g=pg, trim_front=28)):
        e = check(codec, B, Q, lens, c, False, shifts=(0, 5), what="poly-G ascii")
        check(codec, code, Q, lens, c, True, shifts=(0, 9), what="poly-G codes")
    e = expected(B, Q, lens, crit(poly_g=pg), False)
    n0 = len(body)
    assert list(e["length"][:3]) == [n0 + pg - 1, n0, n0] and list(e["length"][3:6]) == [n0 + 7, n0 + 2 * pg, n0 + 7]
    assert list(e["length"][6:11]) == [0, 0, pg - 1, 0, 0] and list(e["length"][11:14]) == [n0, n0 + 5, n0] and e["length"][14] == 8 + n0
    # a run that reaches into trim_tail: the bases trimmed off do not count towards it
    e = expected(B, Q, lens, crit(poly_g=pg, trim_tail=2), False)
    assert e["length"][1] == n0 + pg - 2 and e["length"][2] == n0
    # in code mode an ASCII 'G' is no G, and in ASCII mode code 2 is none
    check(codec, B, Q, lens, crit(poly_g=2), True, what="ascii bytes judged as codes")
    check(codec, code, Q, lens, crit(poly_g=2), False, what="codes judged as ascii")


# ---------------------------------------------------------------- test 4: every reason at equality
def check_reasons(codec):
    L = 40
    rows = []                                                               # (bases, scores, expected why with REASONS)

    def row(b, q, why):
        assert len(b) == len(q)
        rows.append((b, q, why))
    alt = b"ACGT" * 10
    row(alt[:20], [30] * 20, 0); row(alt[:19], [30] * 19, SHORT)                                   # min_len 20
    row(b"NN" + alt[:30], [30] * 32, 0); row(b"NNn" + alt[:30], [30] * 33, MANY_N)                   # max_n 2
    row(alt[:20], [25] * 20, 0); row(alt[:20], [25] * 19 + [24], MEANQ)                             # min_mean_q 25: 500 against 499
    row(alt[:20], [30] * 16 + [14] * 4, 0); row(alt[:21], [30] * 16 + [14] * 5, LOWQ)                # qual_q 15, 20 %: 4 of 20 (400 <= 400), 5 of 21 (500 > 420)
    row(alt[:20], [30] * 15 + [15] * 5, 0)                                                          # a score of qual_q itself is not low
    row(b"A" * 13 + b"CACACACA", [30] * 21, 0); row(b"A" * 14 + b"CACACAC", [30] * 21, COMPLEX)     # 40 % of 20 neighbours: 8 transitions against 7
    row(b"A" * 20, [10] * 19 + [14], MEANQ + LOWQ + COMPLEX); row(b"NNNNN" + b"A" * 10, [10] * 15, SHORT + MANY_N + MEANQ + LOWQ + COMPLEX)
    c = crit(min_len=20, max_n=2, min_mean_q=25, qual_q=15, max_lowq_pct=20, min_complexity_pct=40)
    B = np.array([np.frombuffer(b.ljust(L, b"N"), np.uint8) for b, _, _ in rows]); Q = np.array([q + [0] * (L - len(q)) for _, q, _ in rows], np.uint8)
    lens = np.array([len(b) for b, _, _ in rows], np.int32)
    e = check(codec, B, Q, lens, c, False, shifts=(0, 3), what="reasons")
    assert list(e["why"]) == [w for _, _, w in rows], (list(e["why"]), [w for _, _, w in rows])
    # n of 0 and of 1: an empty window fails no mean and no complexity rule, and neither does a single base; only min_len sees them
    lens2 = np.array([0, 1, 0, 1], np.int32); B2 = np.full((4, 16), 65, np.uint8); Q2 = np.zeros((4, 16), np.uint8); Q2[1, 0] = 25; Q2[3, 0] = 24
    c2 = crit(min_mean_q=25, min_complexity_pct=100)
    e = check(codec, B2, Q2, lens2, c2, False, what="n of 0 and 1")
    assert list(e["why"]) == [0, 0, 0, MEANQ] and list(e["keep"]) == [1, 1, 1, 0]
    e = check(codec, B2, Q2, lens2, crit(min_len=1, min_mean_q=25, min_complexity_pct=100), False, what="n of 0 and 1, min_len 1")
    assert list(e["why"]) == [SHORT, 0, SHORT, MEANQ]
    # a threshold no byte reaches, and the products in 64 bits
    big = crit(min_mean_q=0xFFFFFFFF, qual_q=0xFFFFFFFF, max_lowq_pct=100, cut_flags=FRONT, cut_window=1000, cut_mean_q=0xFFFFFFFF)
    e = check(codec, B, Q, lens, big, False, what="32-bit thresholds")
    assert set(e["length"]) == {0} and set(e["why"]) == {0}


# ---------------------------------------------------------------- test 5: empty and degenerate
def check_degenerate(codec):
    for L in (16, 40):
        B, Q, lens = random_rows(70, L, 77 + L, codes=True)
        allc = STEPS[-1][1]
        for c in (crit(trim_front=L, trim_tail=0), crit(trim_front=L // 2, trim_tail=L - L // 2), crit(trim_front=0xFFFFFFFF, trim_tail=0xFFFFFFFF),
                  dict(allc, trim_front=L // 2, trim_tail=L // 2), dict(allc, max_len=2), crit(cut_flags=FRONT | TAIL, cut_window=9, cut_mean_q=15, max_len=3),
                  crit(max_len=0xFFFFFFFF), crit(cut_flags=RIGHT, cut_window=1, cut_mean_q=0), crit(cut_flags=FRONT | RIGHT | TAIL, cut_window=1000, cut_mean_q=256)):
            check(codec, B, Q, lens, c, True, shifts=(0, 15), what="degenerate")
        check(codec, B, Q, np.zeros(70, np.int32), allc, True, what="all lengths 0")
        e = check(codec, B, Q, np.zeros(70, np.int32), crit(), True, what="all lengths 0, no criterion")
        assert e["summary"]["n_kept"] == 70 and e["summary"]["bases_in"] == 0


# ---------------------------------------------------------------- test 6: a long row, naturally
def check_long_rows(codec):
    L, w = 70000, 4
    Q = np.zeros((3, L), np.uint8); B = np.random.default_rng(6).integers(0, 5, (3, L)).astype(np.uint8)
    lens = np.array([L, L - 1, 35002], np.int32)
    mid = 34999
    for kind, flag in (("front", FRONT), ("tail", TAIL)):
        Q[:] = 0
        Q[0, mid:mid + w] = 20; Q[1, L - 1 - w:L - 1] = 20; Q[2, 35002 - w:35002] = 20; Q[2, 35002:] = 99
        c = crit(cut_flags=flag, cut_window=w, cut_mean_q=20)
        e = check(codec, B, Q, lens, c, True, shifts=(0, 5), paths=(None,), what="long " + kind)
        want = [(mid, L - mid), (L - 1 - w, w), (35002 - w, w)] if kind == "front" else [(0, mid + w), (0, L - 1), (0, 35002)]
        assert [(int(a), int(m)) for a, m in zip(e["start"], e["length"])] == want
    Q[:] = 20
    Q[0, mid + w - 1] = 19; Q[1, L - 2] = 19; Q[2, 35001] = 19
    e = check(codec, B, Q, lens, crit(cut_flags=RIGHT, cut_window=w, cut_mean_q=20), True, shifts=(0, 11), paths=(None,), what="long right")
    assert list(e["length"]) == [mid, L - 1 - w, 35002 - w]
    allc = dict(STEPS[-1][1], max_len=0, cut_window=1000, cut_mean_q=20)
    Q[:] = np.random.default_rng(7).integers(15, 27, (3, L)).astype(np.uint8)
    check(codec, B, Q, lens, allc, True, shifts=(1,), paths=(None,), what="long, everything")


# ---------------------------------------------------------------- tests 7 and 8: outputs and summary
def check_outputs_and_summary(codec):
    B, Q, lens = random_rows(700, 150, 8, codes=False)
    c = STEPS[-1][1]
    e = expected(B, Q, lens, c, False)
    assert 0 < e["summary"]["n_kept"] < 700 and all(e["summary"][f] > 0 for f in FIELDS), e["summary"]
    dev = W.DevRows(codec, B, Q, lens, shift=3)
    try:
        for path in (None, "general"):
            codec.set_option("RFQ_JUDGE", path)
            for outputs in ("k", "s", "l", "w", "m", "", "kslwm"):
                out, summ, raw = run(codec, dev, c, False, outputs)
                compare(out, summ, e, "outputs %r" % outputs)
            out2, summ2, raw2 = run(codec, dev, c, False, "kslwm")
            assert raw2 == raw and summ2 == summ, "the same call on the same context gave other bytes"
    finally:
        codec.set_option("RFQ_JUDGE", None)
        dev.free()
    # rows without bases or without qualities, where no criterion needs them: their counts are 0
    dev = W.DevRows(codec, B, Q, lens)
    try:
        zb = np.zeros_like(B)
        for c2, args, ref in ((crit(min_len=50, min_mean_q=20, qual_q=10, max_lowq_pct=50), (dev.n, dev.L, None, dev.quals, dev.lens), (zb, Q)),
                              (crit(min_len=50, max_n=3, poly_g=3, min_complexity_pct=30), (dev.n, dev.L, dev.bases, None, dev.lens), (B, np.zeros_like(Q)))):
            e2 = expected(ref[0], ref[1], lens, c2, False)
            g = W.Guarded(codec, 16 * dev.n); gk = W.Guarded(codec, dev.n)
            try:
                r = codec.judge_rows(*args, **c2, d_metrics=g.ptr, d_keep=gk.ptr)
                assert g.guards_intact() and gk.guards_intact()
                assert np.array_equal(np.frombuffer(g.body(), np.uint32).reshape(-1, 4), e2["metrics"]) and np.array_equal(np.frombuffer(gk.body(), np.uint8), e2["keep"])
                assert summary_of(r) == e2["summary"]
            finally:
                g.free(); gk.free()
    finally:
        dev.free()


# ---------------------------------------------------------------- test 9: refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens = random_rows(40, 33, 9, codes=True)
    check(codec, B, Q, lens, STEPS[-1][1], True, paths=(None,), what="after a refusal")


def check_host_refusals(codec):
    from repaq_amd import RfqError
    n, L = 40, 32
    B, Q, lens = random_rows(n, L, 10, codes=False)
    dev = W.DevRows(codec, B, Q, lens)
    buf = codec.dev_put(b"\0" * 4096); b = buf.value
    try:
        rows = dev.judge_args()

        def at(p, k):
            return C.c_void_p(p.value + k)
        J = codec.judge_rows
        calls = (("unknown cut_flags bits", lambda: J(*rows, cut_flags=8, cut_window=4)),
                 ("cut flag with cut_window 0", lambda: J(*rows, cut_flags=FRONT, cut_window=0)),
                 ("cut flag with cut_window 1001", lambda: J(*rows, cut_flags=TAIL, cut_window=1001)),
                 ("max_lowq_pct 101", lambda: J(*rows, qual_q=10, max_lowq_pct=101)),
                 ("min_complexity_pct 101", lambda: J(*rows, min_complexity_pct=101)),
                 ("bad base_mode", lambda: J(*rows, base_mode=2)),
                 ("row_len 0", lambda: J(n, 0, dev.bases, dev.quals, dev.lens)),
                 ("no quals with a cut flag", lambda: J(n, L, dev.bases, None, dev.lens, cut_flags=RIGHT, cut_window=4)),
                 ("no quals with min_mean_q", lambda: J(n, L, dev.bases, None, dev.lens, min_mean_q=1)),
                 ("no quals with qual_q", lambda: J(n, L, dev.bases, None, dev.lens, qual_q=1)),
                 ("no bases with poly_g", lambda: J(n, L, None, dev.quals, dev.lens, poly_g=3)),
                 ("no bases with max_n", lambda: J(n, L, None, dev.quals, dev.lens, max_n=0)),
                 ("no bases with min_complexity_pct", lambda: J(n, L, None, dev.quals, dev.lens, min_complexity_pct=1)),
                 ("misaligned d_lens", lambda: J(n, L, dev.bases, dev.quals, at(dev.lens, 2))),
                 ("misaligned d_start", lambda: J(*rows, d_start=C.c_void_p(b + 1))),
                 ("misaligned d_len", lambda: J(*rows, d_len=C.c_void_p(b + 2))),
                 ("misaligned d_metrics", lambda: J(*rows, d_metrics=C.c_void_p(b + 3))),
                 ("keep on bases", lambda: J(*rows, d_keep=at(dev.bases, n * L - 1))),
                 ("why ends in quals", lambda: J(*rows, d_why=C.c_void_p(dev.quals.value - n + 1))),
                 ("start on lens", lambda: J(*rows, d_start=dev.lens)),
                 ("len on the last length", lambda: J(*rows, d_len=at(dev.lens, 4 * (n - 1)))),
                 ("metrics on quals", lambda: J(*rows, d_metrics=at(dev.quals, 16))))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3, (what, ei.value)
            _good(codec)
        # (a cut_window is not looked at without a cut flag, outputs of the caller's own that lie on nothing are taken, and so are no rows at all)
        assert J(*rows, cut_window=5000, d_keep=C.c_void_p(b), d_start=C.c_void_p(b + 64), d_metrics=C.c_void_p(b + 1024)).n_rows == n
        assert summary_of(J(0, 0, None, None, None, cut_flags=FRONT, cut_window=4)) == dict.fromkeys(FIELDS, 0)
    finally:
        dev.free(); codec.dev_free(buf)


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "middle", "last")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    for L, n in ((24, 300), (300, 9), (1100, 5)):
        B, Q, lens = random_rows(n, L, 11, codes=True)
        row = dict(first=0, middle=n // 2, last=n - 1)[where]
        lens[row] = -1 if value == "negative" else L + 1
        lens[(row + 1) % n] = L                                              # (a good row beside it)
        dev = W.DevRows(codec, B, Q, lens, shift=1)
        try:
            for path in (None, "general"):
                codec.set_option("RFQ_JUDGE", path)
                for outputs in ("", "kslwm"):
                    with R.pytest_raises(RfqError) as ei:
                        run(codec, dev, STEPS[-1][1], True, outputs)
                    assert ei.value.code == -3 and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                codec.set_option("RFQ_JUDGE", None)
                _good(codec)
        finally:
            codec.set_option("RFQ_JUDGE", None)
            dev.free()


# ---------------------------------------------------------------- test 10: composition
COMPOSE = crit(trim_front=1, poly_g=6, cut_flags=FRONT | TAIL, cut_window=4, cut_mean_q=18, min_len=40, max_n=12, min_mean_q=18, qual_q=12, max_lowq_pct=45,
               min_complexity_pct=20)


def compose_text(pairs=600, seed=12):
    """two FASTQ texts of `pairs` records: lengths 20 .. 151, scores that fall off towards the ends, G tails, N runs, reads of one base"""
    rng = np.random.default_rng(seed)
    out = [[], []]
    for k in range(pairs):
        for m in (0, 1):
            l = int(rng.choice((151, 151, 150, 120, 76, 45, 20)))
            (B, Q, _) = random_rows(3, l, int(rng.integers(1 << 30)), codes=False)              # (row 0 is a read of the full length)
            if rng.random() < 0.85:
                Q = np.minimum(Q.astype(np.int32) + 14, 41).astype(np.uint8)
            s = bytes(B[0]).upper(); q = bytes(np.minimum(Q[0], 60) + 33)
            out[m].append(b"@run7.%d %d/%d\n" % (k + 1, k + 1, m + 1) + s + b"\n+\n" + q + b"\n")
    return out


def compose_expected(recs, c, min_len):
    """the two texts the criteria leave: every record judged by judge_row, a pair stands or falls together, a window shorter than min_len falls"""
    verdicts = []
    for rec in recs:
        name, s, _, q = rec.split(b"\n")[:4]
        k, a, m, _, _ = judge_row(list(s), [x - 33 for x in q], len(s), c, False)
        verdicts.append((k and m >= min_len, name, s[a:a + m], q[a:a + m]))
    out = [[], []]
    for i in range(0, len(verdicts), 2):
        if verdicts[i][0] and verdicts[i + 1][0]:
            for m in (0, 1):
                _, name, s, q = verdicts[i + m]
                out[m].append(name + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(out[0]), b"".join(out[1]), len(out[0])


def check_composition(codec):
    import _select as S
    from repaq_amd import PE_TWO_FILES
    t1, t2 = compose_text()
    fq1, fq2 = b"".join(t1), b"".join(t2)
    recs = [x for pair in zip(t1, t2) for x in pair]
    w1, w2, kept = compose_expected(recs, COMPOSE, COMPOSE["min_len"])
    assert 100 < kept < 500, kept
    _, B, Q, lens, names = codec.text_rows_bytes(fq1, fq2, paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    assert n == 1200
    dev = W.DevRows(codec, B, Q, lens, names)
    gk, gs, gl = W.Guarded(codec, n), W.Guarded(codec, 4 * n), W.Guarded(codec, 4 * n)
    bufs = []
    try:
        j = codec.judge_rows(n, 160, dev.bases, dev.quals, dev.lens, **COMPOSE, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
        assert j.n_rows == n and all(g.guards_intact() for g in (gk, gs, gl))
        sel = dict(d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr, pairs=True, min_len=COMPOSE["min_len"])
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
        for g in (gk, gs, gl):
            g.free()
        for p in bufs:
            codec.dev_free(p)
    return fq1, fq2, w1, w2


# ---------------------------------------------------------------- test 11: the seams of the shared walk
JR_ITER = 8                                                                   # (enc/rows_judge.h)
_walk_sets = {}


def walk_sets(L, counts):
    """per count: rows, mode and the reference under every criterion at once - made once per row length, shared by the default and the general path"""
    if L not in _walk_sets:
        _walk_sets[L] = [(random_rows(n, L, 31 * L + n, codes=n % 2 == 1), n % 2 == 1) for n in counts]
        _walk_sets[L] = [(rows, codes, expected(*rows, STEPS[-1][1], codes)) for rows, codes in _walk_sets[L]]
    return _walk_sets[L]


def check_walk(codec, label):
    L, path, counts = W.walk_case(label, JR_ITER)
    for (B, Q, lens), codes, e in walk_sets(L, counts):
        check(codec, B, Q, lens, STEPS[-1][1], codes, shifts=(len(lens) % 16,), paths=(path,), e=e, what="walk L %d n %d" % (L, len(lens)))


def check_walk_bad_length(codec):
    """a bad length in the last row of a workgroup's first row behind its last step: the refusal names it"""
    from repaq_amd import RfqError
    for L in (256, 272):
        n = 256 // (16 if L <= 256 else 64) * JR_ITER + 1
        B, Q, lens = random_rows(n, L, 5, codes=True)
        lens[n - 1] = L + 1
        dev = W.DevRows(codec, B, Q, lens)
        try:
            with R.pytest_raises(RfqError) as ei:
                run(codec, dev, STEPS[-1][1], True)
            assert ei.value.code == -3 and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
        finally:
            dev.free()
