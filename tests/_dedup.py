"""Shared helpers of the rfq_dedup_rows tests (tests/test_emu_dedup.py on the SIMT interpreter, tests/test_gpu_dedup.py on the MI355X).

Nothing expected comes from the code under test: expected() is a Python dict from a unit's key bytes - per row the key length and the bytes in front of it, as
include/rfq_hip.h defines them - to the list of its members; the representative, the class sizes, the histogram and the summary are read off that dict.  Every
comparison is exact integer equality.  Every output goes into a _rows.Guarded buffer of exactly as many entries as the call may write, and the guards are checked
after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R

FIELDS = ("n_units", "n_candidates", "n_classes", "n_dups", "max_class", "bases_in", "bases_kept")
OPTION = "RFQ_DEDUP"
PATHS = (None, "collide")


# ---------------------------------------------------------------- the reference
def unit_key(Bb, lens, u, nr, key_len):
    """the key of unit u: per row (k, the k bytes in front) - Bb: the rows as bytes objects"""
    key = []
    for g in range(nr * u, nr * u + nr):
        l = int(lens[g]); k = min(l, key_len) if key_len else l
        key.append((k, Bb[g][:k]))
    return tuple(key)


def expected(B, Q, lens, pairs=False, key_len=0, best=False, cand=None, hist_len=0):
    """what rfq_dedup_rows must write and report: keep [n], dup_of [U], count [U], hist [hist_len] as numpy arrays and the summary as a dict"""
    n = len(lens); nr = 2 if pairs else 1; U = n // nr
    Bb = [bytes(r) for r in np.ascontiguousarray(B)]
    keep = np.zeros(n, np.uint8); dup_of = np.full(U, -1, np.int32); count = np.zeros(U, np.uint32); hist = np.zeros(hist_len, np.uint64)
    s = dict.fromkeys(FIELDS, 0); s["n_units"] = U
    classes = {}
    for u in range(U):
        rows = range(nr * u, nr * u + nr)
        if cand is not None and not all(int(cand[g]) for g in rows):
            continue
        s["n_candidates"] += 1; s["bases_in"] += sum(int(lens[g]) for g in rows)
        classes.setdefault(unit_key(Bb, lens, u, nr, key_len), []).append(u)
    for key, members in classes.items():
        rep = members[0]                                                     # (members are in ascending order)
        if best:
            def score(u):
                return sum(int(Q[nr * u + i, :key[i][0]].astype(np.int64).sum()) for i in range(nr))
            top = max(score(u) for u in members)
            rep = min(u for u in members if score(u) == top)
        c = len(members)
        for u in members:
            dup_of[u] = rep
        count[rep] = c; keep[nr * rep:nr * rep + nr] = 1
        s["n_classes"] += 1; s["max_class"] = max(s["max_class"], c); s["bases_kept"] += sum(int(lens[g]) for g in range(nr * rep, nr * rep + nr))
        if hist_len:
            hist[min(c, hist_len) - 1] += 1
    s["n_dups"] = s["n_candidates"] - s["n_classes"]
    return dict(keep=keep, dup_of=dup_of, count=count, hist=hist, summary=s, classes=classes)


def summary_of(r):
    return {f: int(getattr(r, f)) for f in FIELDS}


NAMES = dict(k="keep", d="dup_of", c="count", h="hist")
DTYPES = dict(k=np.uint8, d=np.int32, c=np.uint32, h=np.uint64)
OUT_ARGS = dict(k="d_keep", d="d_dup_of", c="d_count", h="d_hist")


def dev_rows(codec, B, Q, lens, cand=None, shift=0):
    return W.DevRows(codec, B, Q, lens, shift=shift, cand=(cand, np.uint8))


def run(codec, dev, pairs=False, key_len=0, best=False, hist_len=0, outputs="kdch"):
    """one rfq_dedup_rows into Guarded buffers of exactly the entries the call may write; returns (dict of numpy outputs, summary dict, raw bytes of the outputs)"""
    n = dev.n; U = n // 2 if pairs else n
    if not hist_len:
        outputs = outputs.replace("h", "")
    sizes = dict(k=n, d=4 * U, c=4 * U, h=8 * hist_len)
    g = {o: W.Guarded(codec, sizes[o]) for o in outputs}
    try:
        r = codec.dedup_rows(*dev.judge_args(), pairs=pairs, key_len=key_len, best_qual=best, hist_len=hist_len, d_in=dev.cand, **{OUT_ARGS[o]: g[o].ptr for o in outputs})
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
    assert summ["n_dups"] == summ["n_candidates"] - summ["n_classes"]


def check(codec, B, Q, lens, pairs=False, key_len=0, best=False, cand=None, hist_len=0, shifts=(0,), paths=PATHS, outputs="kdch", what="", no_quals=False):
    """the call equals the reference, at every shift and under both values of the option; returns the reference"""
    e = expected(B, Q, lens, pairs, key_len, best, cand, hist_len)
    for shift in shifts:
        dev = dev_rows(codec, B, None if no_quals else Q, lens, cand, shift)
        try:
            for path in paths:
                codec.set_option(OPTION, path)
                out, summ, _ = run(codec, dev, pairs, key_len, best, hist_len, outputs)
                compare(out, summ, e, "%s shift %d option %s:" % (what, shift, path or "default"))
        finally:
            codec.set_option(OPTION, None)
            dev.free()
    return e


def sizes_of(e):
    return sorted(len(m) for m in e["classes"].values())


# ---------------------------------------------------------------- test 1: planted classes
ROW_LENS = (1, 15, 16, 17, 100, 150, 256, 257, 300, 1024, 1025, 1500)
PLANTED = (1000, 40, 17, 3, 2) + (1,) * 200                                  # 205 classes (<= 256: probing under collide is quadratic), 1262 units
ALPHA = np.frombuffer(b"ACGTNacgtn", np.uint8)


def planted(L, pairs, seed, sizes=PLANTED):
    """units in classes of the given sizes: every class has its own lengths (12 .. L, mixed within the batch; the first classes take L) and key bytes, every member
    its own noise behind its reads and its own scores; shuffled, then members of the largest class are put at both ends of the batch"""
    rng = np.random.default_rng(seed); nr = 2 if pairs else 1
    U = sum(sizes); n = nr * U
    cls = np.repeat(np.arange(len(sizes)), sizes)
    clen = rng.integers(min(L, 12), L + 1, (len(sizes), nr)); clen[:3] = L; clen[3] = max(L - 1, 0)          # (12 bytes and more: no two classes share a key by chance)
    cbytes = ALPHA[rng.integers(0, len(ALPHA), (len(sizes), nr, L))]
    order = rng.permutation(U)
    big = np.nonzero(cls[order] == 0)[0]
    for dst, src in ((0, big[0]), (1, big[1]), (U - 1, big[-1]), (U - 2, big[-2])):
        order[[dst, src]] = order[[src, dst]]
    cls = cls[order]
    lens = clen[cls].reshape(n).astype(np.int32)
    B = cbytes[cls].reshape(n, L)
    noise = rng.integers(0, 256, (n, L), dtype=np.uint8)
    B = np.where(np.arange(L)[None, :] < lens[:, None], B, noise).astype(np.uint8)
    Q = rng.integers(0, 42, (n, L)).astype(np.uint8)
    return B, Q, lens


def check_planted(codec, L, pairs):
    i = ROW_LENS.index(L)
    B, Q, lens = planted(L, pairs, 100 * L + pairs)
    e = None
    for j, (best, path) in enumerate(((False, None), (True, None), (False, "collide"), (True, "collide"))):
        hist_len = (1, 8, 1024)[(i + j + pairs) % 3]
        e = check(codec, B, Q, lens, pairs=pairs, best=best, hist_len=hist_len, paths=(path,), what="planted L %d pairs %d best %d" % (L, pairs, best))
    if L >= 15:                                                              # (keys of one byte fall together by chance: the dict still says what is right)
        assert sizes_of(e) == sorted(PLANTED), sizes_of(e)[-6:]
    u = e["dup_of"][0]
    assert e["summary"]["max_class"] >= 1000 and e["dup_of"][len(e["dup_of"]) - 1] == u and e["count"][u] >= 1000


# ---------------------------------------------------------------- test 2: near misses
def _rand(rng, n, L):
    return ALPHA[rng.integers(0, 4, (n, L))].astype(np.uint8)                # (ACGT: a changed byte is then always another byte below)


def check_every_position(codec):
    """a row, its copy, and the row with one byte changed at position p, for every p of a 300-byte key: one class of two, 300 of one"""
    rng = np.random.default_rng(21); L = 300
    X = _rand(rng, 1, L)[0]
    B = np.tile(X, (L + 2, 1))
    for p in range(L):
        B[2 + p, p] = ord("N")
    lens = np.full(L + 2, L, np.int32); Q = np.zeros_like(B)
    e = check(codec, B, Q, lens, shifts=(0, 3), what="one byte changed")
    assert sizes_of(e) == [1] * L + [2] and e["dup_of"][1] == 0
    # the same in R2 of a pair, and in R1
    P = np.tile(np.concatenate([X, X[::-1]]), (L + 2, 1)).reshape(-1, L)     # pairs (X, reversed X)
    for mate in (0, 1):
        B2 = P.copy()
        for p in range(L):
            B2[2 * (2 + p) + mate, p] = ord("N")
        e = check(codec, B2, np.zeros_like(B2), np.full(2 * (L + 2), L, np.int32), pairs=True, what="one byte changed in mate %d" % mate)
        assert sizes_of(e) == [1] * L + [2]


def check_lengths_and_padding(codec):
    rng = np.random.default_rng(22); L = 100
    A = _rand(rng, 1, L)[0]
    rows, lens = [], []
    # a proper prefix of a row, the longer row's bytes still behind it: not a copy; beside the true copy of each
    rows += [A, A, A, A]; lens += [L, 60, L, 60]
    # rows that differ only at positions >= their length: padding 0, 255, noise -> copies
    C1 = _rand(rng, 1, L)[0]
    for pad in (0, 255, None):
        r = C1.copy(); r[37:] = rng.integers(0, 256, L - 37) if pad is None else pad
        rows.append(r); lens.append(37)
    # upper against lower case: not copies
    U1 = _rand(rng, 1, L)[0]
    rows += [U1, U1 | 0x20, U1]; lens += [50, 50, 50]
    # a single lower-case letter in the last key byte
    lo = U1.copy(); lo[49] |= 0x20
    rows.append(lo); lens.append(50)
    B = np.array(rows, np.uint8); lens = np.array(lens, np.int32)
    e = check(codec, B, np.zeros_like(B), lens, shifts=(0, 1), what="lengths and padding")
    assert list(e["dup_of"]) == [0, 1, 0, 1, 4, 4, 4, 7, 8, 7, 10], list(e["dup_of"])
    # all-empty rows: one class, whatever lies in them
    Bz = rng.integers(0, 256, (33, 20), dtype=np.uint8)
    for pairs in (False, True):
        e = check(codec, Bz[:32], np.zeros((32, 20), np.uint8), np.zeros(32, np.int32), pairs=pairs, hist_len=8, what="empty rows")
        assert sizes_of(e) == [16 if pairs else 32] and e["summary"]["bases_in"] == 0


def check_key_len(codec):
    rng = np.random.default_rng(23); L = 120
    for key_len in (1, 16, 17, 50):
        A = _rand(rng, 1, L)[0]
        rows = [A.copy() for _ in range(7)]; lens = [L, L, L, L, 90, 10, 10]
        rows[1][key_len:] = _rand(rng, 1, L - key_len)[0]                     # differs only beyond key_len: a copy
        rows[2][key_len - 1] = ord("N")                                      # differs at key_len - 1: not a copy
        rows[3][key_len] = ord("N")                                          # differs at key_len: a copy
        # row 4: another length, still >= key_len: a copy.  rows 5, 6: shorter than key_len (for 16, 17, 50): their own lengths count - copies of each other only
        B = np.array(rows, np.uint8); lens = np.array(lens, np.int32)
        Q = rng.integers(0, 42, B.shape).astype(np.uint8)
        for best in (False, True):
            e = check(codec, B, Q, lens, key_len=key_len, best=best, what="key_len %d" % key_len)
            short = 0 if key_len <= 10 else 5
            assert [int(e["dup_of"][i] == e["dup_of"][0]) for i in range(7)] == [1, 1, 0, 1, 1, int(short == 0), int(short == 0)], (key_len, list(e["dup_of"]))
            assert e["dup_of"][5] == e["dup_of"][6]
        # a key_len beyond every read is no key_len
        assert np.array_equal(check(codec, B, Q, lens, key_len=L + 5)["dup_of"], expected(B, Q, lens)["dup_of"])


def check_pairs(codec):
    rng = np.random.default_rng(24); L = 64
    X, Y, Z = _rand(rng, 3, L)
    AB = _rand(rng, 1, 40)[0]

    def row(b):
        r = np.full(L, 255, np.uint8); r[:len(b)] = b
        return r, len(b)
    units = [(X, Y), (X, Y),                # a pair and its copy
             (X, Z),                        # equal in R1 only
             (Z, Y),                        # equal in R2 only
             (Y, X),                        # the mates swapped
             (AB[:30], AB[30:]), (AB[:20], AB[20:]), (AB[:30], AB[30:]),      # (AB, C) against (A, BC): the bytes of the two mates back to back are the same
             (X[:0], Y), (X[:0], Y), (Y, X[:0])]                              # an empty mate
    rows, lens = zip(*(row(b) for u in units for b in u))
    B = np.array(rows, np.uint8); lens = np.array(lens, np.int32)
    e = check(codec, B, np.zeros_like(B), lens, pairs=True, shifts=(0, 7), what="pairs")
    assert list(e["dup_of"]) == [0, 0, 2, 3, 4, 5, 6, 5, 8, 8, 10], list(e["dup_of"])
    # without pairs the same rows are judged one by one
    e = check(codec, B, np.zeros_like(B), lens, pairs=False, what="the pairs' rows alone")
    assert e["dup_of"][2] == 0 and e["dup_of"][3] == 1 and e["dup_of"][8] == 1 and e["dup_of"][9] == 0


# ---------------------------------------------------------------- test 3: best quality
def check_best_quality(codec):
    rng = np.random.default_rng(25); L, m = 90, 5
    A = _rand(rng, 1, L)[0]
    for pairs in (False, True):
        nr = 2 if pairs else 1
        for where in (0, m // 2, m - 1, "tie", "beyond"):
            B = np.tile(A, (m * nr + nr, 1)); B[-1, 0] = ord("N")            # the class and a stranger behind it
            lens = np.full(len(B), 70, np.int32)
            Q = np.full(B.shape, 20, np.uint8)
            if where == "tie":
                Q[1 * nr, 3] = 30; Q[3 * nr + nr - 1, 69] = 30                # members 1 and 3 lead with equal sums: the lower index
                want = 1
            elif where == "beyond":
                Q[2 * nr:, 70:] = 41; Q[4 * nr, 70] = 255                    # scores that differ only behind the key: equal sums, the lowest index
                want = 0
            else:
                Q[where * nr + nr - 1, 69] = 21                              # one point more, in the last key byte of the unit's last row
                want = where
            e = check(codec, B, Q, lens, pairs=pairs, best=True, hist_len=8, what="best at %s" % (where,))
            assert list(e["dup_of"][:m]) == [want] * m and e["count"][want] == m, (where, list(e["dup_of"]))
            assert list(check(codec, B, Q, lens, pairs=pairs, best=False)["dup_of"][:m]) == [0] * m
    # with pairs the score is over both mates: R1 alone would choose member 0, R2 alone member 1, the sum member 2
    B = np.tile(A, (6, 1)); lens = np.full(6, 70, np.int32); Q = np.full(B.shape, 10, np.uint8)
    Q[0, :10] = 20; Q[3, :10] = 20; Q[4, :7] = 20; Q[5, :7] = 20
    e = check(codec, B, Q, lens, pairs=True, best=True, what="both mates' scores")
    assert list(e["dup_of"]) == [2, 2, 2]
    # a key_len cuts the window of the score too
    Q = np.full(B.shape, 10, np.uint8); Q[2, 30] = 40; Q[4, 16] = 11
    e = check(codec, B, Q, lens, best=True, key_len=17, what="score under key_len")
    assert list(e["dup_of"]) == [4] * 6
    # scores of 255 over a full row of 1500: the largest sums the small kernels and the tiled one meet
    B = np.tile(_rand(rng, 1, 1500)[0], (4, 1)); Q = np.full(B.shape, 255, np.uint8); Q[0, 1499] = 254; Q[1, 0] = 254; Q[3, 700] = 254
    e = check(codec, B, Q, np.full(4, 1500, np.int32), best=True, what="large scores")
    assert list(e["dup_of"]) == [2] * 4


# ---------------------------------------------------------------- test 4: candidates
def check_candidates(codec):
    B, Q, lens = planted(150, False, 26, sizes=(40, 17, 3, 2) + (1,) * 30)
    n = len(lens)
    e0 = expected(B, Q, lens)
    rng = np.random.default_rng(27)
    cand = np.ones(n, np.uint8)
    reps = np.nonzero(e0["keep"])[0]
    cand[reps[e0["count"][reps] == 40]] = 0                                  # the would-be representative of a class
    cand[e0["dup_of"] == reps[e0["count"][reps] == 17][0]] = 0               # a whole class
    cand[reps[e0["count"][reps] == 1][:5]] = 0                               # five classes of one
    cand[np.nonzero(e0["dup_of"] == reps[e0["count"][reps] == 3][0])[0][1:]] = 0      # all of a class but its first
    cand[cand != 0] = rng.integers(1, 256, int((cand != 0).sum()))           # (any non-zero byte counts)
    for best in (False, True):
        e = check(codec, B, Q, lens, cand=cand, best=best, hist_len=8, shifts=(0, 1), what="candidates")
        out = cand == 0
        assert e["summary"]["n_candidates"] == n - int(out.sum()) and (e["dup_of"][out] == -1).all() and not e["keep"][out].any() and not e["count"][out].any()
        assert sizes_of(e) == sorted((39, 2, 1) + (1,) * 25)
    # pairs: one mate out takes the unit out, and its bases out of bases_in
    B, Q, lens = planted(100, True, 28, sizes=(9, 4, 2) + (1,) * 10)
    cand = np.ones(len(lens), np.uint8)
    cand[0] = 0; cand[7] = 0; cand[20] = cand[21] = 0
    e = check(codec, B, Q, lens, pairs=True, cand=cand, hist_len=4, what="one mate out")
    assert list(e["dup_of"][[0, 3, 10]]) == [-1, -1, -1] and e["summary"]["n_candidates"] == len(lens) // 2 - 3
    assert not e["keep"][[0, 1, 6, 7, 20, 21]].any()
    # nobody is a candidate
    e = check(codec, B, Q, lens, pairs=True, cand=np.zeros(len(lens), np.uint8), hist_len=4, what="no candidates")
    assert e["summary"] == dict(dict.fromkeys(FIELDS, 0), n_units=len(lens) // 2)


# ---------------------------------------------------------------- test 5: shapes and outputs
def check_shapes_and_outputs(codec):
    for L in (33, 100, 150, 160, 300, 1100):                                      # (no multiples of 16 but one: rows at their own alignment at every shift)
        for pairs in (False, True):
            B, Q, lens = planted(L, pairs, 29 + L, sizes=(20, 5, 2) + (1,) * 40)
            check(codec, B, Q, lens, pairs=pairs, best=True, hist_len=8, shifts=(0, 1, 7, 15), what="shifts L %d" % L)
            check(codec, B, Q, lens, pairs=pairs, best=False, shifts=(7,), no_quals=True, what="no quality rows in FIRST")
    B, Q, lens = planted(150, False, 30, sizes=(20, 5, 2) + (1,) * 40)
    e = expected(B, Q, lens, hist_len=8)
    dev = dev_rows(codec, B, Q, lens, shift=3)
    try:
        for path in PATHS:
            codec.set_option(OPTION, path)
            for outputs in ("k", "d", "c", "h", "", "kdch"):
                out, summ, raw = run(codec, dev, hist_len=8, outputs=outputs)
                assert set(out) == set(outputs)
                compare(out, summ, e, "outputs %r" % outputs)
            out2, summ2, raw2 = run(codec, dev, hist_len=8)
            assert raw2 == raw and summ2 == summ, "the same call on the same context gave other bytes"
    finally:
        codec.set_option(OPTION, None)
        dev.free()
    # a histogram length is not looked at without a histogram
    assert check(codec, B, Q, lens, hist_len=0)["summary"]["n_classes"] == 43
    for n in (0, 1, 2):
        for pairs in (False, True):
            if pairs and n == 1:
                continue
            Bn = np.tile(B[:1], (n, 1)).reshape(n, 150)
            e = check(codec, Bn, Q[:n], np.full(n, 150, np.int32), pairs=pairs, best=True, hist_len=3, what="n_rows %d" % n)
            assert e["summary"]["n_classes"] == (1 if n else 0) and list(e["hist"]) == [int(n == 1 or (pairs and n == 2)), int(n == 2 and not pairs), 0]
    r = codec.dedup_rows(0, 0, None, None, None, pairs=True, best_qual=True)
    assert summary_of(r) == dict.fromkeys(FIELDS, 0)


# ---------------------------------------------------------------- test 6: state
def check_state(codec, make_codec):
    """a large batch, then a small one whose keys all occurred in the large one, on one context: the small one's result is a fresh context's - nothing of the
    first table is left -, and the same call twice gives the same bytes"""
    B, Q, lens = planted(40, False, 31, sizes=(1000, 42, 17, 3, 2) + (16,) * 246)      # 5000 units in 251 classes
    assert len(lens) == 5000
    pick = np.array([0, 17, 4999, 0, 300, 17, 2500, 2501, 300, 4999])
    Bs, Qs, ls = B[pick], Q[pick], lens[pick]
    es = expected(Bs, Qs, ls, best=True, hist_len=8)
    fresh = make_codec()
    try:
        d = dev_rows(fresh, Bs, Qs, ls)
        try:
            want = run(fresh, d, best=True, hist_len=8)
        finally:
            d.free()
    finally:
        fresh.close()
    compare(want[0], want[1], es, "a fresh context:")
    big, small = dev_rows(codec, B, Q, lens), dev_rows(codec, Bs, Qs, ls)
    try:
        first = run(codec, big, best=True, hist_len=8)
        compare(first[0], first[1], expected(B, Q, lens, best=True, hist_len=8), "the large batch:")
        got = run(codec, small, best=True, hist_len=8)
        assert got[2] == want[2] and got[1] == want[1], "a small batch behind a large one differs from a fresh context's"
        again = run(codec, big, best=True, hist_len=8)
        assert again[2] == first[2] and again[1] == first[1], "the same call on the same context gave other bytes"
    finally:
        big.free(); small.free()


# ---------------------------------------------------------------- test 7: refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens = planted(33, True, 9, sizes=(6, 3) + (1,) * 11)
    check(codec, B, Q, lens, pairs=True, best=True, hist_len=4, paths=(None,), what="after a refusal")


def check_host_refusals(codec):
    from repaq_amd import RfqError
    B, Q, lens = planted(32, False, 10, sizes=(20, 10) + (1,) * 10)
    n, L = B.shape
    cand = np.ones(n, np.uint8)
    dev = dev_rows(codec, B, Q, lens, cand)
    buf = codec.dev_put(b"\0" * 16384); b = buf.value
    try:
        rows = dev.judge_args()

        def at(p, k):
            return C.c_void_p(p.value + k)
        D = codec.dedup_rows
        calls = (("pairs takes rows in pairs", lambda: D(n - 1, L, dev.bases, dev.quals, dev.lens, pairs=True)),
                 ("unknown mode", lambda: D(*rows, mode=2)),
                 ("unknown mode", lambda: D(*rows, mode=-1)),
                 ("needs rows->d_quals", lambda: D(n, L, dev.bases, None, dev.lens, best_qual=True)),
                 ("row_len must be >= 1", lambda: D(n, 0, dev.bases, dev.quals, dev.lens)),
                 ("at most 2^22", lambda: D(n, (1 << 22) + 1, dev.bases, dev.quals, dev.lens)),
                 ("null d_lens / d_bases", lambda: D(n, L, None, dev.quals, dev.lens)),
                 ("null d_lens / d_bases", lambda: D(n, L, dev.bases, dev.quals, None)),
                 ("4-byte aligned", lambda: D(n, L, dev.bases, dev.quals, at(dev.lens, 2))),
                 ("4-byte aligned", lambda: D(*rows, d_dup_of=C.c_void_p(b + 1))),
                 ("4-byte aligned", lambda: D(*rows, d_count=C.c_void_p(b + 2))),
                 ("8-byte aligned", lambda: D(*rows, d_hist=C.c_void_p(b + 4), hist_len=8)),
                 ("hist_len must be", lambda: D(*rows, d_hist=C.c_void_p(b), hist_len=1025)),
                 ("hist_len must be", lambda: D(*rows, hist_len=1025)),
                 ("hist_len must be", lambda: D(*rows, d_hist=C.c_void_p(b), hist_len=0)),
                 ("d_keep overlaps the input rows->d_bases", lambda: D(*rows, d_keep=at(dev.bases, n * L - 1))),
                 ("d_keep overlaps the input d_in", lambda: D(*rows, d_in=dev.cand, d_keep=dev.cand)),
                 ("d_dup_of overlaps the input rows->d_lens", lambda: D(*rows, d_dup_of=dev.lens)),
                 ("d_count overlaps the input rows->d_lens", lambda: D(*rows, d_count=at(dev.lens, 4 * (n - 1)))),
                 ("d_count overlaps the input rows->d_quals", lambda: D(*rows, best_qual=True, d_count=at(dev.quals, 16))),
                 ("d_hist overlaps the input rows->d_bases", lambda: D(*rows, d_hist=at(dev.bases, -56), hist_len=8)),
                 ("too many units", lambda: D((1 << 31) - 1, 1, dev.bases, dev.quals, dev.lens)),
                 ("too many units", lambda: D((1 << 32) - 2, 1, dev.bases, dev.quals, dev.lens, pairs=True)),
                 ("pairs must be 0 or 1", lambda: codec._check(_raw_pairs(codec, rows, 2))))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3 and what in ei.value.message, (what, ei.value)
            _good(codec)
        # (outputs of the caller's own that lie on nothing are taken; a quality row may be written over where no score is asked for; no rows at all are no error)
        assert D(*rows, d_keep=C.c_void_p(b), d_dup_of=C.c_void_p(b + 1024), d_count=C.c_void_p(b + 4096), d_hist=C.c_void_p(b + 8192), hist_len=1024).n_units == n
        assert D(*rows, best_qual=False, d_keep=dev.quals).n_units == n
        assert summary_of(D(0, 0, None, None, None, pairs=True, hist_len=3)) == dict.fromkeys(FIELDS, 0)
    finally:
        dev.free(); codec.dev_free(buf)


def _raw_pairs(codec, rows, pairs):
    """the C call with a `pairs` the Python wrapper cannot express"""
    from repaq_amd import _capi as A
    n, L, pb, pq, pl = rows
    ri = codec._rows_in(n, L, pb, pq, pl, None, 0, None, False, 0)
    a = A.DedupRowsArgs(pairs, 0, 0, 0, None, None, None, None, None); r = A.DedupRowsResult()
    return codec._L.rfq_dedup_rows(codec._h, C.byref(ri), C.byref(a), C.byref(r))


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "last", "pair_r1", "pair_r2")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    for L, n in ((24, 300), (300, 10), (1100, 6)):
        rng = np.random.default_rng(11)
        B = _rand(rng, n, L); Q = np.zeros_like(B); lens = rng.integers(0, L + 1, n).astype(np.int32)
        pairs = where.startswith("pair")
        row = dict(first=0, last=n - 1, pair_r1=n // 2 & ~1, pair_r2=(n // 2 & ~1) + 1)[where]
        lens[row] = -1 if value == "negative" else L + 1
        for cand in (None, (np.arange(n) != row).astype(np.uint8)):          # (every row is judged, candidate or not)
            dev = dev_rows(codec, B, Q, lens, cand, shift=1)
            try:
                for path in PATHS:
                    codec.set_option(OPTION, path)
                    for outputs in ("", "kdch"):
                        with R.pytest_raises(RfqError) as ei:
                            run(codec, dev, pairs=pairs, best=True, hist_len=4, outputs=outputs)
                        assert ei.value.code == -3 and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                    codec.set_option(OPTION, None)
                    _good(codec)
            finally:
                codec.set_option(OPTION, None)
                dev.free()
    # two bad rows: the first is named
    lens = np.full(n, L, np.int32); lens[1] = -5; lens[4] = L + 1
    dev = dev_rows(codec, B, Q, lens)
    try:
        with R.pytest_raises(RfqError) as ei:
            run(codec, dev)
        assert "first such row: 1)" in ei.value.message
    finally:
        dev.free()
    _good(codec)


def check_option(codec, reset):
    from repaq_amd import RfqError
    assert OPTION in codec.option_names() and codec.get_option(OPTION) == ""
    codec.set_option(OPTION, "collide")
    assert codec.get_option(OPTION) == "collide"
    reset(codec)
    assert codec.get_option(OPTION) == ""
    for bad in ("general", "Collide", "1"):
        with R.pytest_raises(RfqError):
            codec.set_option(OPTION, bad)
    assert codec.get_option(OPTION) == ""


# ---------------------------------------------------------------- test 8: composition
def compose_text(pairs=260, seed=13):
    """_judge.compose_text's records with copies planted: every fifth pair comes again once or twice further on, under a name of its own"""
    import _judge as J
    t1, t2 = J.compose_text(pairs=pairs, seed=seed)
    rng = np.random.default_rng(seed)
    out = [[], []]
    k = 0
    for i in rng.permutation(np.concatenate([np.arange(pairs), np.arange(0, pairs, 5), np.arange(0, pairs, 10)])):
        k += 1
        for m, t in ((0, t1), (1, t2)):
            out[m].append(b"@copy%d/%d\n" % (k, m + 1) + t[i].split(b"\n", 1)[1])
    return out


def compose_expected(t1, t2, c):
    """the two texts judge -> dedup -> select leave: a pair whose two reads pass the judge is a candidate, of the candidates with identical reads (whole, untrimmed)
    the first stays, trimmed to the judge's windows"""
    import _judge as J
    seen = set(); out = [[], []]; dups = 0
    for r1, r2 in zip(t1, t2):
        v = []
        for rec in (r1, r2):
            name, s, _, q = rec.split(b"\n")[:4]
            k, a, m, _, _ = J.judge_row(list(s), [x - 33 for x in q], len(s), c, False)
            v.append((k, name, s, s[a:a + m], q[a:a + m]))
        if not (v[0][0] and v[1][0]):
            continue
        key = (v[0][2], v[1][2])
        if key in seen:
            dups += 1
            continue
        seen.add(key)
        for m in (0, 1):
            out[m].append(v[m][1] + b"\n" + v[m][3] + b"\n+\n" + v[m][4] + b"\n")
    return b"".join(out[0]), b"".join(out[1]), len(out[0]), dups


def check_composition(codec):
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    t1, t2 = compose_text()
    fq1, fq2 = b"".join(t1), b"".join(t2)
    c = J.COMPOSE
    w1, w2, kept, dups = compose_expected(t1, t2, c)
    assert kept > 50 and dups > 20, (kept, dups)
    _, B, Q, lens, names = codec.text_rows_bytes(fq1, fq2, paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    dev = W.DevRows(codec, B, Q, lens, names)
    gk, gs, gl, gd = W.Guarded(codec, n), W.Guarded(codec, 4 * n), W.Guarded(codec, 4 * n), W.Guarded(codec, n)
    bufs = []
    try:
        codec.judge_rows(n, 160, dev.bases, dev.quals, dev.lens, **c, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
        d = codec.dedup_rows(n, 160, dev.bases, dev.quals, dev.lens, pairs=True, d_in=gk.ptr, d_keep=gd.ptr)
        assert all(g.guards_intact() for g in (gk, gs, gl, gd))
        assert int(d.n_classes) == kept and int(d.n_dups) == dups
        sel = dict(d_keep=gd.ptr, d_start=gs.ptr, d_len=gl.ptr, pairs=True, min_len=c["min_len"])
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
        for g in (gk, gs, gl, gd):
            g.free()
        for p in bufs:
            codec.dev_free(p)


# ---------------------------------------------------------------- test 12: the seams of the shared walk
DD_ITER = 8                                                                   # (enc/rows_dedup.h)


def check_walk(codec, label):
    """FIRST over rows and BEST_QUAL over pairs, the last unit a copy of the first with the higher scores: a class of two whose representative FIRST and BEST_QUAL
    choose differently (from two units on)"""
    L, _, counts = W.walk_case(label, DD_ITER)
    for U in counts:
        for pairs, best in ((False, False), (True, True)):
            nr = 2 if pairs else 1; n = nr * U
            rng = np.random.default_rng(31 * L + n)
            B = _rand(rng, n, L); Q = rng.integers(0, 40, (n, L)).astype(np.uint8); lens = rng.integers(min(L, 12), L + 1, n).astype(np.int32)
            if U > 1:
                B[n - nr:] = B[:nr]; lens[n - nr:] = lens[:nr]; Q[n - nr:] = 41
            e = check(codec, B, Q, lens, pairs=pairs, best=best, hist_len=4, shifts=(n % 16,), paths=(None,), what="walk L %d units %d pairs %d" % (L, U, pairs))
            if U > 1:
                assert e["dup_of"][U - 1] == e["dup_of"][0] == (U - 1 if best else 0) and e["summary"]["n_dups"] >= 1


def check_walk_bad_length(codec):
    """a bad length in the last row, a workgroup's first unit behind its last step: the refusal names it"""
    from repaq_amd import RfqError
    for L in (256, 272):
        n = 256 // (16 if L <= 256 else 64) * DD_ITER + 1
        rng = np.random.default_rng(5)
        B = _rand(rng, n, L); lens = rng.integers(0, L + 1, n).astype(np.int32)
        lens[n - 1] = L + 1
        dev = dev_rows(codec, B, np.zeros_like(B), lens)
        try:
            with R.pytest_raises(RfqError) as ei:
                run(codec, dev, best=True, hist_len=4)
            assert ei.value.code == -3 and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
        finally:
            dev.free()
