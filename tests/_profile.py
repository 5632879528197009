"""Shared helpers of the rfq_profile_rows tests (tests/test_emu_profile.py on the SIMT interpreter, tests/test_gpu_profile.py on the MI355X).

Nothing expected comes from the code under test: expected() is plain numpy written from the rules of include/rfq_hip.h - a loop over the rows; every row gives the
table cells of its window's positions and its own bins, which are counted at the end - and shares nothing with the product.  Every comparison is exact integer
equality.  Every table goes into a _rows.Guarded buffer of exactly as many entries as the call may write, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R

OPTION = "RFQ_PROFILE"
PATHS = (None, "general")
TABLES = ("base_cnt", "base_qsum", "qual_hist", "len_hist", "meanq_hist", "gc_hist")
FIELDS = ("counted", "bases", "qsum", "q20", "q30", "gc", "other")
GC_BINS = 101
WG_PER_CU = 3                                                                 # (enc/rows_profile.h: PF_WG_PER_CU)
EMU_CUS = 4                                                                   # (tests/emu/include/hip/hip_runtime.h: hipDeviceGetAttribute)

CLS_CODE = np.full(256, 4, np.int64); CLS_CODE[:4] = np.arange(4)
CLS_ASCII = np.full(256, 4, np.int64)
for _k, _c in enumerate(b"ACGT"):
    CLS_ASCII[_c] = CLS_ASCII[_c | 0x20] = _k


# ---------------------------------------------------------------- the reference
def shapes(M, cycles, qbins, len_bins):
    return dict(base_cnt=(M, cycles, 5), base_qsum=(M, cycles, 5), qual_hist=(M, cycles, qbins), len_hist=(M, len_bins), meanq_hist=(M, qbins), gc_hist=(M, GC_BINS))


def expected(B, Q, lens, codes, pairs=False, keep=None, start=None, length=None, cycles=1, qbins=1, len_bins=1):
    """what rfq_profile_rows must write and report: the six tables as uint64 arrays and the summary as a dict (B or Q None: the fields they feed are 0)"""
    M = 2 if pairs else 1; n = len(lens)
    cls_of = CLS_CODE if codes else CLS_ASCII
    sh = shapes(M, cycles, qbins, len_bins)
    t = {k: np.zeros(sh[k], np.uint64) for k in TABLES}
    s = {f: [0] * M for f in FIELDS}; s["n_rows"] = n; s["max_len"] = 0
    base_ix, base_q, qh_ix = [], [], []
    for i in range(n):
        if keep is not None and not int(keep[i]):
            continue
        m = i & 1 if pairs else 0
        a = int(start[i]) if start is not None else 0
        w = int(length[i]) if length is not None else int(lens[i]) - a
        cyc = np.minimum(np.arange(w), cycles - 1) + m * cycles
        q = Q[i, a:a + w].astype(np.int64) if Q is not None else np.zeros(w, np.int64)
        c = cls_of[B[i, a:a + w]] if B is not None else None
        qsum = int(q.sum())
        s["counted"][m] += 1; s["bases"][m] += w; s["qsum"][m] += qsum; s["q20"][m] += int((q >= 20).sum()); s["q30"][m] += int((q >= 30).sum())
        s["max_len"] = max(s["max_len"], w)
        t["len_hist"][m, min(w, len_bins - 1)] += 1
        if w and Q is not None:
            t["meanq_hist"][m, min(qsum // w, qbins - 1)] += 1
        qh_ix.append(cyc * qbins + np.minimum(q, qbins - 1))
        if c is not None:
            gc = int(((c == 1) | (c == 2)).sum()); acgt = int((c < 4).sum())
            s["gc"][m] += gc; s["other"][m] += w - acgt
            if acgt:
                t["gc_hist"][m, 100 * gc // acgt] += 1
            base_ix.append(cyc * 5 + c); base_q.append(q)
    if base_ix:
        ix = np.concatenate(base_ix); qq = np.concatenate(base_q)
        t["base_cnt"] = np.bincount(ix, minlength=M * cycles * 5).astype(np.uint64).reshape(sh["base_cnt"])
        t["base_qsum"] = np.bincount(ix, weights=qq, minlength=M * cycles * 5).astype(np.uint64).reshape(sh["base_qsum"])      # (sums far below 2^53: exact)
    if qh_ix and Q is not None:
        t["qual_hist"] = np.bincount(np.concatenate(qh_ix), minlength=M * cycles * qbins).astype(np.uint64).reshape(sh["qual_hist"])
    t["summary"] = s
    return t


def summary_of(r, M):
    s = {f: [int(getattr(r, f)[m]) for m in range(M)] for f in FIELDS}
    assert all(int(getattr(r, f)[1]) == 0 for f in FIELDS) or M == 2, "mate 1 holds counts without pairs"
    s["n_rows"] = int(r.n_rows); s["max_len"] = int(r.max_len)
    return s


def dev_rows(codec, B, Q, lens, keep=None, start=None, length=None, shift=0):
    return W.DevRows(codec, B, Q, lens, shift=shift, keep=(keep, np.uint8), start=(start, np.int32), length=(length, np.int32))


def run(codec, dev, codes, pairs=False, cycles=1, qbins=1, len_bins=1, tables=TABLES, no_bases=False):
    """one rfq_profile_rows into Guarded buffers of exactly the entries the call may write; returns (dict of numpy tables, summary dict, raw bytes of the tables)"""
    M = 2 if pairs else 1
    sh = shapes(M, cycles, qbins, len_bins)
    g = {k: W.Guarded(codec, 8 * int(np.prod(sh[k]))) for k in tables}
    try:
        r = codec.profile_rows(dev.n, dev.L, None if no_bases else dev.bases, dev.quals, dev.lens, codes=codes, pairs=pairs, d_keep=dev.keep, d_start=dev.start,
                               d_len=dev.length, cycles=cycles, qbins=qbins, len_bins=len_bins, **{"d_" + k: g[k].ptr for k in tables})
        assert all(x.guards_intact() for x in g.values()), "a guard around a table was written"
        raw = {k: x.body() for k, x in g.items()}
        return {k: np.frombuffer(raw[k], np.uint64).reshape(sh[k]) for k in tables}, summary_of(r, M), raw
    finally:
        for x in g.values():
            x.free()


def compare(out, summ, e, what=""):
    for k, got in out.items():
        want = e[k]
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want); i = tuple(int(x) for x in bad[0])
            raise AssertionError("%s %s differs in %d of %d cells, first %r: got %d, want %d" % (what, k, len(bad), want.size, i, got[i], want[i]))
    assert summ == e["summary"], (what, {k: (summ[k], e["summary"][k]) for k in summ if summ[k] != e["summary"][k]})


def check(codec, B, Q, lens, codes, pairs=False, keep=None, start=None, length=None, cycles=None, qbins=64, len_bins=None, shifts=(0,), paths=PATHS, tables=TABLES,
          what="", e=None):
    """the call equals the reference, at every shift and on both paths; returns the reference"""
    L = B.shape[1]
    cycles = L if cycles is None else cycles; len_bins = L + 1 if len_bins is None else len_bins
    if e is None:
        e = expected(B, Q, lens, codes, pairs, keep, start, length, cycles, qbins, len_bins)
    for shift in shifts:
        dev = dev_rows(codec, B, Q, lens, keep, start, length, shift)
        try:
            for path in paths:
                codec.set_option(OPTION, path)
                out, summ, _ = run(codec, dev, codes, pairs, cycles, qbins, len_bins, tables)
                compare(out, summ, e, "%s shift %d path %s:" % (what, shift, path or "default"))
        finally:
            codec.set_option(OPTION, None)
            dev.free()
    return e


# ---------------------------------------------------------------- rows
ASCII_ALPHA = np.frombuffer(b"AACCGGTTNacgtnRYKM.", np.uint8)                  # (lower case counts as its base; N, IUPAC letters and the rest are other)
CODE_ALPHA = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 255], np.uint8)


def random_rows(n, L, seed, codes, lo=0):
    """n rows of stride L: lengths lo .. L (the first two L and 0 where there are that many), bases of every class, scores 0 .. 45 with 0 and 255 among them, noise
    behind the reads"""
    rng = np.random.default_rng(seed)
    alpha = CODE_ALPHA if codes else ASCII_ALPHA
    B = alpha[rng.integers(0, len(alpha), (n, L))]
    Q = rng.integers(0, 46, (n, L)).astype(np.uint8)
    Q[rng.random((n, L)) < 0.02] = 255; Q[rng.random((n, L)) < 0.02] = 0
    lens = rng.integers(lo, L + 1, n).astype(np.int32)
    if n > 0:
        lens[0] = L
    if n > 2:
        lens[2] = 0
    return np.ascontiguousarray(B), Q, lens


def random_windows(lens, seed, full=0.3):
    """a window inside every read: some whole, some empty, the rest anywhere"""
    rng = np.random.default_rng(seed); n = len(lens)
    start = (rng.random(n) * (lens + 1)).astype(np.int32); start = np.minimum(start, lens)
    length = (rng.random(n) * (lens - start + 1)).astype(np.int32)
    whole = rng.random(n) < full
    start[whole] = 0; length[whole] = lens[whole]
    length[rng.random(n) < 0.1] = 0
    return start.astype(np.int32), length.astype(np.int32)


# ---------------------------------------------------------------- test 1: every table and the summary
ROW_LENS = (1, 15, 16, 17, 150)


def check_tables(codec, L, pairs, codes):
    n = 70
    B, Q, lens = random_rows(n, L, 1000 * L + 2 * pairs + codes, codes)
    check(codec, B, Q, lens, codes, pairs=pairs, shifts=(0, 3), what="tables L %d pairs %d codes %d" % (L, pairs, codes))
    rng = np.random.default_rng(L)
    keep = (rng.random(n) < 0.7).astype(np.uint8); start, length = random_windows(lens, L + 1)
    check(codec, B, Q, lens, codes, pairs=pairs, keep=keep, start=start, length=length, shifts=(1,), what="tables under a triple L %d pairs %d codes %d" % (L, pairs, codes))


def step_units(L, pairs, n_cu):
    """units (rows of a mate) a step of the whole grid takes on the common path: beyond it a workgroup takes a second step (rfq_profile_rows' grid: WG_PER_CU
    workgroups per compute unit, shared among the mates)"""
    R = 16 if L <= 256 else 4
    return R * max(1, WG_PER_CU * n_cu // (2 if pairs else 1))


def check_walk(codec, label, n_cu):
    """the unit counts around a wave, a step and a workgroup of the shared walk (one step each here: the grid grows first), and around the counts at which the
    per-workgroup step count becomes 2 and 3 - with pairs per mate, which share the grid"""
    L, path, counts = W.walk_case(label, 1)
    cases = [(U, bool(k & 1)) for k, U in enumerate(counts)]
    if path is None and L <= 1024 and len(counts) > 3:
        S, S2 = step_units(L, False, n_cu), step_units(L, True, n_cu)
        cases += [(S, False), (S + 1, False), (2 * S + 5, False), (S2 + 1, True)]
    for k, (U, pairs) in enumerate(cases):
        codes = bool(k & 2)
        n = U * (2 if pairs else 1)
        B, Q, lens = random_rows(n, L, 31 * L + n, codes, lo=min(L, 12))
        start = length = keep = None
        if k % 3 == 0:
            start, length = random_windows(lens, n); keep = (np.arange(n) % 5 != 1).astype(np.uint8)
        check(codec, B, Q, lens, codes, pairs=pairs, keep=keep, start=start, length=length, qbins=42, shifts=(n % 16,), paths=(path,),
              what="walk L %d units %d pairs %d" % (L, U, pairs))


# ---------------------------------------------------------------- test 2: windows
def check_windows(codec):
    L, n = 100, 48
    B, Q, lens = random_rows(n, L, 5, False, lo=40)
    Q[3, :] = 0; Q[4, :] = 255; Q[5, ::2] = 255; Q[5, 1::2] = 0
    for pairs in (False, True):
        # every row at one start: 0, 1, 15, 16, 17, l - 1 (the window to the end of the read, and windows given); windows of 0; a window across a 16-byte group
        for s0 in (0, 1, 15, 16, 17, "l-1"):
            start = (lens - 1 if s0 == "l-1" else np.minimum(s0, lens)).astype(np.int32); start = np.maximum(start, 0).astype(np.int32)
            check(codec, B, Q, lens, False, pairs=pairs, start=start, what="start %s, to the end" % (s0,))
            length = np.minimum(lens - start, np.arange(n) % 23).astype(np.int32)     # (0 .. 22 positions: empty windows, windows inside a group and across one)
            check(codec, B, Q, lens, False, pairs=pairs, start=start, length=length, shifts=(5,), what="start %s, short windows" % (s0,))
        check(codec, B, Q, lens, False, pairs=pairs, length=np.zeros(n, np.int32), what="all windows empty")
        s14 = np.minimum(14, lens).astype(np.int32)
        check(codec, B, Q, lens, False, pairs=pairs, start=s14, length=np.minimum(4, lens - s14).astype(np.int32), what="a window across a 16-byte group")
        # windows longer than cycles: the overflow row is exact; cycles 1; cycles beyond the stride
        start, length = random_windows(lens, 9)
        for cycles in (1, 2, 10, 16, 17, 99, L + 50):
            e = check(codec, B, Q, lens, False, pairs=pairs, start=start, length=length, cycles=cycles, what="cycles %d" % cycles)
            assert e["summary"]["max_len"] > 17
            if 1 < cycles <= 17:
                assert int(e["base_cnt"][:, cycles - 1].sum()) > int(e["base_cnt"][:, 0].sum()), "the overflow row holds no more than a cycle"
        # score bins 1, 42, 256 with the scores 0 and 255 present; one length bin
        for qbins in (1, 2, 42, 255, 256):
            e = check(codec, B, Q, lens, False, pairs=pairs, start=start, length=length, qbins=qbins, shifts=(2,), what="qbins %d" % qbins)
            assert int(e["qual_hist"][..., qbins - 1].sum()) > 0 and int(e["qual_hist"][..., 0].sum()) > 0
        for len_bins in (1, 2, 50, L + 1, 1 << 20):
            check(codec, B, Q, lens, False, pairs=pairs, start=start, length=length, len_bins=len_bins, tables=("len_hist",) if len_bins > 4096 else TABLES,
                  what="len_bins %d" % len_bins)
    # tables beyond a workgroup's LDS go the long way by themselves: the same cells
    B, Q, lens = random_rows(40, 300, 6, True)
    check(codec, B, Q, lens, True, cycles=300, qbins=256, paths=(None,), what="tables beyond the LDS")
    check(codec, B, Q, lens, True, cycles=65536, qbins=2, tables=("base_cnt", "qual_hist"), paths=(None,), what="cycles 65536")


# ---------------------------------------------------------------- test 3: masks
def check_masks(codec):
    L, n = 60, 90
    for codes in (False, True):
        B, Q, lens = random_rows(n, L, 7 + codes, codes)
        rng = np.random.default_rng(8)
        keep = rng.choice(np.array([0, 0, 2, 7, 128, 255], np.uint8), n)     # (any non-zero byte counts)
        start, length = random_windows(lens, 9)
        for pairs in (False, True):
            e = check(codec, B, Q, lens, codes, pairs=pairs, keep=keep, start=start, length=length, what="mask bytes other than 1")
            assert sum(e["summary"]["counted"]) == int((keep != 0).sum())
            e = check(codec, B, Q, lens, codes, pairs=pairs, keep=np.zeros(n, np.uint8), start=start, length=length, what="all dropped")
            assert e["summary"] == dict({f: [0] * (1 + pairs) for f in FIELDS}, n_rows=n, max_len=0) and not any(int(e[k].sum()) for k in TABLES)
            check(codec, B, Q, lens, codes, pairs=pairs, keep=keep, what="a mask without windows")
            check(codec, B, Q, lens, codes, pairs=pairs, length=length // 2, what="lengths without starts")


# ---------------------------------------------------------------- test 4: outputs
def check_outputs(codec):
    L, n = 150, 64
    B, Q, lens = random_rows(n, L, 10, True)
    start, length = random_windows(lens, 11)
    kw = dict(pairs=True, cycles=L, qbins=42, len_bins=L + 1)
    e = expected(B, Q, lens, True, True, None, start, length, L, 42, L + 1)
    dev = dev_rows(codec, B, Q, lens, None, start, length, shift=3)
    try:
        for path in PATHS:
            codec.set_option(OPTION, path)
            for tables in [(k,) for k in TABLES] + [(), TABLES]:
                out, summ, raw = run(codec, dev, True, tables=tables, **kw)
                assert set(out) == set(tables)
                compare(out, summ, e, "tables %r" % (tables,))
            out2, summ2, raw2 = run(codec, dev, True, **kw)
            assert raw2 == raw and summ2 == summ, "the same call on the same context gave other bytes"
            assert "profile:rows" in [name for name, _ in codec.timings()]
    except BaseException:
        dev.free()
        raise
    finally:
        codec.set_option(OPTION, None)
    # without quality rows the tables that need none: the score fields are 0; without base rows the same of gc and other
    devq = W.DevRows(codec, B, None, lens, keep=(None, np.uint8), start=(start, np.int32), length=(length, np.int32))
    try:
        eq = expected(B, None, lens, True, True, None, start, length, L, 42, L + 1)
        for path in PATHS:
            codec.set_option(OPTION, path)
            out, summ, _ = run(codec, devq, True, tables=("base_cnt", "len_hist", "gc_hist"), **kw)
            compare(out, summ, eq, "no quality rows")
            assert summ["qsum"] == [0, 0] and summ["q20"] == [0, 0]
            eb = expected(None, Q, lens, True, True, None, start, length, L, 42, L + 1)
            out, summ, _ = run(codec, dev, True, tables=("qual_hist", "len_hist", "meanq_hist"), no_bases=True, **kw)
            compare(out, summ, eb, "no base rows")
            assert summ["gc"] == [0, 0] and summ["other"] == [0, 0]
    finally:
        codec.set_option(OPTION, None)
        devq.free(); dev.free()


# ---------------------------------------------------------------- test 5: state
def check_state(codec, make_codec, others):
    """two different calls on one context, then the first again: equal tables; a profile between an encode, a decode and a dedup (others(codec) runs them) equals the
    same call on a fresh context; no rows zero the tables"""
    B1, Q1, l1 = random_rows(500, 150, 12, True); B2, Q2, l2 = random_rows(90, 40, 13, False)
    s1, w1 = random_windows(l1, 14)
    d1, d2 = dev_rows(codec, B1, Q1, l1, None, s1, w1), dev_rows(codec, B2, Q2, l2)
    kw1 = dict(pairs=True, cycles=150, qbins=64, len_bins=151); kw2 = dict(cycles=7, qbins=3, len_bins=2)
    fresh = make_codec()
    try:
        f1 = dev_rows(fresh, B1, Q1, l1, None, s1, w1)
        try:
            want = run(fresh, f1, True, **kw1)
        finally:
            f1.free()
    finally:
        fresh.close()
    compare(want[0], want[1], expected(B1, Q1, l1, True, True, None, s1, w1, 150, 64, 151), "a fresh context:")
    try:
        first = run(codec, d1, True, **kw1)
        other = run(codec, d2, False, **kw2)
        compare(other[0], other[1], expected(B2, Q2, l2, False, False, None, None, None, 7, 3, 2), "the second call:")
        again = run(codec, d1, True, **kw1)
        assert first[2] == want[2] and first[1] == want[1] and again[2] == first[2] and again[1] == first[1], "something is left of an earlier call"
        others(codec)
        between = run(codec, d1, True, **kw1)
        assert between[2] == want[2] and between[1] == want[1], "a call between other kinds of calls differs from a fresh context's"
    finally:
        d1.free(); d2.free()
    # no rows: the tables are zeroed (the guarded buffers start as 0xA5), the result is all zero
    for pairs in (False, True):
        M = 1 + pairs
        sh = shapes(M, 9, 5, 4)
        g = {k: W.Guarded(codec, 8 * int(np.prod(sh[k]))) for k in TABLES}
        try:
            r = codec.profile_rows(0, 0, None, None, None, pairs=pairs, cycles=9, qbins=5, len_bins=4, **{"d_" + k: g[k].ptr for k in TABLES})
            assert all(x.guards_intact() for x in g.values()) and all(set(x.body()) == {0} for x in g.values())
            assert summary_of(r, M) == dict({f: [0] * M for f in FIELDS}, n_rows=0, max_len=0)
        finally:
            for x in g.values():
                x.free()


def other_calls(codec):
    """an encode, a decode and a dedup on the context"""
    import _oracle as O
    fq1, _ = O.gen(O.NOVA_SE150, 200, seed=3)
    img = codec.encode_bytes(fq1)
    assert codec.decode_bytes(img) == fq1
    B, Q, lens = random_rows(64, 50, 15, False)
    d = W.DevRows(codec, B, Q, lens)
    try:
        assert int(codec.dedup_rows(*d.judge_args()).n_units) == 64
    finally:
        d.free()


# ---------------------------------------------------------------- test 6: agreement inside the family
def check_family(codec):
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    t1, t2 = J.compose_text(pairs=300)
    _, B, Q, lens, _names = codec.text_rows_bytes(b"".join(t1), b"".join(t2), paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    dev = W.DevRows(codec, B, Q, lens)
    gk, gs, gl = W.Guarded(codec, n), W.Guarded(codec, 4 * n), W.Guarded(codec, 4 * n)
    kw = dict(cycles=160, qbins=64, len_bins=161)
    bufs = []
    try:
        j = codec.judge_rows(n, 160, dev.bases, dev.quals, dev.lens, **J.COMPOSE, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
        assert 0 < int(j.n_kept) < n
        for path in PATHS:
            codec.set_option(OPTION, path)
            for pairs in (False, True):
                r = codec.profile_rows(n, 160, dev.bases, dev.quals, dev.lens, pairs=pairs, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
                assert [sum(getattr(r, f)) for f in ("counted", "bases", "qsum", "q20", "q30")] == [int(getattr(j, f)) for f in ("n_kept", "bases_out", "qsum_out", "q20_out", "q30_out")]
                r = codec.profile_rows(n, 160, dev.bases, dev.quals, dev.lens, pairs=pairs)
                assert [sum(getattr(r, f)) for f in ("counted", "bases", "qsum", "q20", "q30")] == [n] + [int(getattr(j, f)) for f in ("bases_in", "qsum_in", "q20_in", "q30_in")]
        codec.set_option(OPTION, None)
        # select_rows' output, profiled with no window == the input profiled under the triple
        sel = dict(d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr, pairs=False, min_len=1)
        q = codec.select_rows(*dev.args(), **sel)
        m, L = int(q.n_rows), 160
        assert m == int(j.n_kept)
        ob, oq, ol = (codec.dev_put(b"\0" * k) for k in (m * L, m * L, 4 * m))
        bufs += [ob, oq, ol]
        codec.select_rows(*dev.args(), row_len=L, out_bases=ob, bases_cap=m * L, out_quals=oq, quals_cap=m * L, out_lens=ol, lens_cap=m, **sel)

        class Sel:
            n, L, bases, quals, lens, keep, start, length = m, 160, ob, oq, ol, None, None, None

        class Src:
            n, L, bases, quals, lens, keep, start, length = dev.n, 160, dev.bases, dev.quals, dev.lens, gk.ptr, gs.ptr, gl.ptr
        for path in PATHS:
            codec.set_option(OPTION, path)
            a, b = run(codec, Sel, False, **kw), run(codec, Src, False, **kw)
            assert a[2] == b[2] and dict(a[1], n_rows=0) == dict(b[1], n_rows=0), "the selected rows' tables differ from the tables under the triple"
            assert int(a[0]["len_hist"].sum()) == m
    finally:
        codec.set_option(OPTION, None)
        dev.free()
        for g in (gk, gs, gl):
            g.free()
        for p in bufs:
            codec.dev_free(p)


# ---------------------------------------------------------------- test 8: refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens = random_rows(40, 33, 9, False)
    check(codec, B, Q, lens, False, pairs=True, qbins=8, paths=(None,), what="after a refusal")


def _raw(codec, rows, **kw):
    """the C call with arguments the Python wrapper cannot express"""
    from repaq_amd import _capi as A
    n, L, pb, pq, pl = rows
    ri = codec._rows_in(n, L, pb, pq, pl, None, 0, None, False, 0)
    a = A.ProfileRowsArgs(**kw); r = A.ProfileRowsResult()
    return codec._L.rfq_profile_rows(codec._h, C.byref(ri), C.byref(a), C.byref(r))


def check_host_refusals(codec):
    from repaq_amd import RfqError
    B, Q, lens = random_rows(32, 32, 10, False)
    n, L = B.shape
    dev = dev_rows(codec, B, Q, lens, np.ones(n, np.uint8), np.zeros(n, np.int32), lens)
    buf = codec.dev_put(b"\0" * (1 << 16)); b = buf.value
    try:
        rows = (n, L, dev.bases, dev.quals, dev.lens)

        def at(p, k):
            return C.c_void_p(p.value + k)
        P = codec.profile_rows
        T = C.c_void_p(b)
        sz = dict(cycles=4, qbins=4, len_bins=4)
        calls = [("pairs must be 0 or 1", lambda: codec._check(_raw(codec, rows, pairs=2))),
                 ("pairs takes rows in pairs", lambda: P(n - 1, L, dev.bases, dev.quals, dev.lens, pairs=True)),
                 ("bad base_mode", lambda: P(*rows, base_mode=7)),
                 ("row_len must be >= 1", lambda: P(n, 0, dev.bases, dev.quals, dev.lens)),
                 ("null d_lens", lambda: P(n, L, dev.bases, dev.quals, None)),
                 ("too many rows", lambda: P(1 << 31, 1, dev.bases, dev.quals, dev.lens)),
                 ("4-byte aligned", lambda: P(n, L, dev.bases, dev.quals, at(dev.lens, 2))),
                 ("4-byte aligned", lambda: P(*rows, d_start=at(dev.start, 1))),
                 ("4-byte aligned", lambda: P(*rows, d_len=at(dev.length, 2))),
                 ("the output d_base_cnt overlaps the output d_base_qsum", lambda: P(*rows, d_base_cnt=T, d_base_qsum=C.c_void_p(b + 8 * 19), **sz)),
                 ("the output d_qual_hist overlaps the output d_gc_hist", lambda: P(*rows, d_gc_hist=T, d_qual_hist=C.c_void_p(b + 800), **sz)),
                 ("the output d_len_hist overlaps the output d_meanq_hist", lambda: P(*rows, d_len_hist=T, d_meanq_hist=T, **sz))]
        for t in ("base_cnt", "base_qsum", "qual_hist"):
            calls += [("cycles must be 1 .. 65536", lambda t=t, c=c: P(*rows, **{"d_" + t: T}, cycles=c, qbins=4)) for c in (0, 65537)]
        for t in ("qual_hist", "meanq_hist"):
            calls += [("qbins must be 1 .. 256", lambda t=t, c=c: P(*rows, **{"d_" + t: T}, cycles=4, qbins=c)) for c in (0, 257)]
        calls += [("len_bins must be 1 .. 2^20", lambda c=c: P(*rows, d_len_hist=T, len_bins=c)) for c in (0, (1 << 20) + 1)]
        calls += [("need rows->d_quals", lambda t=t: P(n, L, dev.bases, None, dev.lens, **{"d_" + t: T}, **sz)) for t in ("base_qsum", "qual_hist", "meanq_hist")]
        calls += [("need rows->d_bases", lambda t=t: P(n, L, None, dev.quals, dev.lens, **{"d_" + t: T}, **sz)) for t in ("base_cnt", "base_qsum", "gc_hist")]
        calls += [("must be 8-byte aligned", lambda t=t: P(*rows, **{"d_" + t: C.c_void_p(b + 4)}, **sz)) for t in TABLES]
        ins = (("rows->d_bases", dev.bases, n * L), ("rows->d_quals", dev.quals, n * L), ("rows->d_lens", dev.lens, 4 * n), ("d_keep", dev.keep, n), ("d_start", dev.start, 4 * n),
               ("d_len", dev.length, 4 * n))
        for k, (what, p, size) in enumerate(ins):
            t = TABLES[k]
            where = C.c_void_p((p.value + size - 1) & ~7)                      # (the table begins in the input's last bytes)
            calls.append(("the output d_%s overlaps the input %s" % (t, what),
                          lambda t=t, where=where: P(*rows, d_keep=dev.keep, d_start=dev.start, d_len=dev.length, **{"d_" + t: where}, **sz)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3 and what in ei.value.message, (what, ei.value)
            _good(codec)
        # (sizes that are not looked at without their tables; tables of the caller's own that lie apart; no rows at all are no error)
        assert int(P(*rows, cycles=0, qbins=0, len_bins=0).n_rows) == n
        assert int(P(*rows, d_len_hist=T, len_bins=3, cycles=70000, qbins=999).n_rows) == n
        assert int(P(*rows, d_base_cnt=T, d_base_qsum=C.c_void_p(b + 8 * 20), d_qual_hist=C.c_void_p(b + 1024), d_gc_hist=C.c_void_p(b + 4096), **sz).n_rows) == n
        assert int(P(0, 0, None, None, None, pairs=True, d_meanq_hist=T, qbins=3).n_rows) == 0
    finally:
        dev.free(); codec.dev_free(buf)


BAD = dict(negative=("lens", -1), row_len_plus_1=("lens", "L+1"), start_negative=("start", -1), len_negative=("length", -2), window_past_the_read=("length", "l+1"),
           sum_beyond_32_bits=("both", 0x7FFFFFFF))
DEVICE_REFUSALS = [(v, row) for v in BAD for row in ("first", "last", "partial_wave")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    arr, v = BAD[value]
    for L, n0 in ((24, 320), (300, 12), (1100, 6)):
        n = n0 + 2 if where == "partial_wave" else n0                       # (n0 fills whole waves of either common-path kernel: 4 / 1 rows a wave)
        B, Q, lens = random_rows(n, L, 11, True)
        start, length = random_windows(lens, 12)
        row = 0 if where == "first" else n - 1
        if arr == "lens":
            lens[row] = L + 1 if v == "L+1" else v
        elif arr == "start":
            start[row] = v
        elif arr == "length":
            length[row] = lens[row] - start[row] + 1 if v == "l+1" else v
        else:
            start[row] = length[row] = v
        lens_kind = arr == "lens"
        for keep in (None, (np.arange(n) != row).astype(np.uint8)):         # (every row is judged, counted or not)
            dev = dev_rows(codec, B, Q, lens, keep, start, length, shift=1)
            try:
                for path in PATHS:
                    codec.set_option(OPTION, path)
                    for tables in ((), TABLES):
                        with R.pytest_raises(RfqError) as ei:
                            run(codec, dev, True, pairs=True, cycles=L, qbins=8, len_bins=L + 1, tables=tables)
                        assert ei.value.code == -3 and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                        assert ("read length" in ei.value.message) == lens_kind and ("window" in ei.value.message) != lens_kind, ei.value
                    codec.set_option(OPTION, None)
                    _good(codec)
            finally:
                codec.set_option(OPTION, None)
                dev.free()
    # a bad window in front of a bad length and behind one: the first row is named, with its own rule
    B, Q, lens = random_rows(40, 50, 13, True)
    for first in ("window", "length"):
        l2 = lens.copy(); start = np.zeros(40, np.int32); length = l2.copy()
        l2[20] = -3; length[20] = 0
        start[7 if first == "window" else 33] = -1
        dev = dev_rows(codec, B, Q, l2, None, start, length)
        try:
            for path in PATHS:
                codec.set_option(OPTION, path)
                with R.pytest_raises(RfqError) as ei:
                    run(codec, dev, True)
                assert ("first such row: 7)" in ei.value.message and "window" in ei.value.message) if first == "window" else \
                       ("first such row: 20)" in ei.value.message and "read length" in ei.value.message), ei.value
        finally:
            codec.set_option(OPTION, None)
            dev.free()
    _good(codec)


def check_option(codec, reset):
    from repaq_amd import RfqError
    assert OPTION in codec.option_names() and codec.get_option(OPTION) == ""
    codec.set_option(OPTION, "general")
    assert codec.get_option(OPTION) == "general"
    reset(codec)
    assert codec.get_option(OPTION) == ""
    for bad in ("collide", "General", "1"):
        with R.pytest_raises(RfqError):
            codec.set_option(OPTION, bad)
    assert codec.get_option(OPTION) == ""
