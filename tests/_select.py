"""Shared helpers of the rfq_select_rows tests (tests/test_emu_select.py on the SIMT interpreter, tests/test_gpu_select.py on the MI355X).

Nothing expected comes from the code under test: the kept rows, their windows, lengths, names, offsets and the three drop counts are computed with numpy on the
host from the inputs (expected()).  Every output goes into a _rows.Guarded buffer of exactly the reported size, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _engine as E
import _oracle as O
import _rows as W
import _rows_enc as R
import _text_rows as T

PAD_B, PAD_Q = 0xA7, 0x51


def expected(B, Q, lens, names, keep=None, start=None, length=None, pairs=False, min_len=1):
    """dict of what rfq_select_rows must report and write (rows as lists of byte strings: the stride is the caller's)"""
    n = len(lens); lens = np.asarray(lens, np.int64)
    st = np.zeros(n, np.int64) if start is None else np.asarray(start, np.int64)
    ln = lens - st if length is None else np.asarray(length, np.int64)
    k = np.ones(n, bool) if keep is None else (np.asarray(keep, np.uint8) != 0)
    short = ln < min_len
    stand = k & ~short
    kept = stand & stand.reshape(-1, 2)[:, ::-1].reshape(-1) if pairs else stand
    idx = np.nonzero(kept)[0]
    e = dict(idx=idx, n_in=n, mask=int((~k).sum()), short=int((k & short).sum()), mate=int((stand & ~kept).sum()),
             lens=ln[idx].astype(np.int32), bases=[bytes(B[i, st[i]:st[i] + ln[i]]) for i in idx], quals=[bytes(Q[i, st[i]:st[i] + ln[i]]) for i in idx],
             names=None if names is None else [names[i] for i in idx])
    e["max_len"] = int(e["lens"].max()) if len(idx) else 0
    e["n_bases"] = int(e["lens"].sum())
    e["names_len"] = sum(map(len, e["names"])) if names is not None else 0
    e["max_name"] = max(map(len, e["names"])) if names is not None and len(idx) else 0
    assert e["n_in"] == len(idx) + e["mask"] + e["short"] + e["mate"]
    return e


def dev_sel(codec, B, Q, lens, names, keep=None, start=None, length=None, shift=0, name_off=None):
    """_rows.DevRows with a selection as its extra inputs: dev.keep / dev.start / dev.length (None: the pointer is NULL)"""
    return W.DevRows(codec, B, Q, lens, names, shift=shift, name_off=name_off, keep=(keep, np.uint8), start=(start, np.int32), length=(length, np.int32))


def sel_of(dev):
    """the selection of a dev_sel() as select_rows takes it"""
    return dict(d_keep=dev.keep, d_start=dev.start, d_len=dev.length)


def out_len(ml, rule):
    """the output stride: None / 0 the longest kept window, 1 one more, "x16" the next multiple of 16 above it, an int > 1 as given"""
    if rule in (None, 0):
        return max(ml, 1)
    if rule == "x16":
        return (ml // 16 + 1) * 16
    return ml + 1 if rule == 1 else int(rule)


def call(codec, B, Q, lens, names, keep=None, start=None, length=None, pairs=False, min_len=1, row_len=None, pad_base=PAD_B, pad_qual=PAD_Q,
         in_shift=0, out_shift=0, outputs="bqlno"):
    """One size query and one rfq_select_rows into Guarded buffers of exactly the reported sizes (_rows.compact_into_guarded), compared with expected().  Returns
    (result, bases, quals, lens, names, raw) - an output not in `outputs` is not asked for and comes back as None; raw: the bytes of every output body."""
    e = expected(B, Q, lens, names, keep, start, length, pairs, min_len)
    dev = dev_sel(codec, B, Q, lens, names, keep, start, length, shift=in_shift)
    if names is None:
        outputs = outputs.replace("n", "").replace("o", "")
    try:
        kw = dict(pairs=pairs, min_len=min_len, **sel_of(dev))
        q = codec.select_rows(*dev.args(), **kw)
        n = len(e["idx"])
        got = (q.n_rows, q.n_bases, q.names_len, q.max_len, q.max_name, q.n_in, q.dropped_mask, q.dropped_short, q.dropped_mate)
        want = (n, e["n_bases"], e["names_len"], e["max_len"], e["max_name"], e["n_in"], e["mask"], e["short"], e["mate"])
        assert got == want, (got, want)
        assert q.n_in == q.n_rows + q.dropped_mask + q.dropped_short + q.dropped_mate

        def rows_differ(kind, g, wantr, bad):
            return "%s rows differ: %d of %d, first %d (input row %d): %r / %r" % (kind, len(bad), n, bad[0], e["idx"][bad[0]], bytes(g[bad[0]][:48]),
                                                                                   bytes(wantr[bad[0]][:48]))
        r, gB, gQ, gL, raw = W.compact_into_guarded(codec, lambda **out: codec.select_rows(*dev.args(), **out, **kw), e, out_len(e["max_len"], row_len),
                                                    pad_base, pad_qual, outputs, out_shift, rows_differ=rows_differ)
        for f in ("n_rows", "n_bases", "names_len", "max_len", "max_name", "n_in", "dropped_mask", "dropped_short", "dropped_mate"):
            assert getattr(r, f) == getattr(q, f), (f, getattr(r, f), getattr(q, f))
        return r, gB, gQ, gL, e["names"], raw
    finally:
        dev.free()


def small_rows(n, L, seed, name_lens=(1, 2, 3), full=False):
    """n rows of stride L with random bytes, lengths 1..L (full: all L), names of the given lengths in turn"""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (n, L), dtype=np.uint8); Q = rng.integers(0, 256, (n, L), dtype=np.uint8)
    lens = np.full(n, L, np.int32) if full else rng.integers(1, L + 1, n).astype(np.int32)
    names = [(b"@%d" % i * 40)[:name_lens[i % len(name_lens)]] for i in range(n)]
    return B, Q, lens, names


# ---------------------------------------------------------------- test 1: identity
def check_identity(codec, label):
    _, fq1, fq2, paired, _ = R.BY_LABEL[label]
    B, Q, lens, names = R.rows_of(fq1, fq2, paired, extra=3, pad=7)
    r, gB, gQ, gL, gN, _ = call(codec, B, Q, lens, names, row_len=B.shape[1])
    assert r.n_in == r.n_rows == len(lens) and gN == names
    inside = np.arange(B.shape[1])[None, :] < lens[:, None]
    assert np.array_equal(np.where(inside, B, PAD_B), gB) and np.array_equal(np.where(inside, Q, PAD_Q), gQ)


# ---------------------------------------------------------------- test 2: windows at every residue
WINDOW_ROW_LENS = (1, 15, 16, 17, 33, 150, 160)
WINDOW_SHIFTS = ((0, 0), (1, 7), (7, 1), (15, 15), (0, 1), (15, 0))


def windows(L):
    """(start, length) over every start in 0..min(17, L), with ends at every residue mod 16 (the first and the last such end) and the full length"""
    out = []
    for s in range(0, min(17, L) + 1):
        ends = {L}
        for r in range(16):
            c = [x for x in range(s, L + 1) if x % 16 == r]
            if c:
                ends |= {c[0], c[-1]}
        out += [(s, x - s) for x in sorted(ends)]
    return out


def check_windows(codec, L):
    win = windows(L)
    assert {(s + w) % 16 for s, w in win} == set(range(min(16, L + 1))) and {s for s, _ in win} == set(range(min(17, L) + 1))
    n = len(win)
    B, Q, lens, names = small_rows(n, L, seed=L, full=True)
    start = np.array([s for s, _ in win], np.int32); length = np.array([w for _, w in win], np.int32)
    for rule in (0, 1, "x16"):
        for in_shift, out_shift in WINDOW_SHIFTS:
            call(codec, B, Q, lens, names, start=start, length=length, min_len=0, row_len=rule, in_shift=in_shift, out_shift=out_shift)
    # d_len NULL: to the end of the read, of reads shorter than the stride too
    lens2 = np.maximum(lens - (np.arange(n) % 3).astype(np.int32), start).astype(np.int32)
    call(codec, B, Q, lens2, names, start=start, min_len=0, row_len="x16")


# ---------------------------------------------------------------- test 3: masks
MASK_ROWS = (0, 1, 2, 255, 256, 257, 2049)


def mask_patterns(n):
    rng = np.random.default_rng(1000 + n)
    pats = {"all": np.ones(n, np.uint8), "none": np.zeros(n, np.uint8), "first": np.zeros(n, np.uint8), "last": np.zeros(n, np.uint8),
            "alternating": (np.arange(n) % 2).astype(np.uint8), "run_over_256": ((np.arange(n) >= 250) & (np.arange(n) < 262)).astype(np.uint8),
            "half": (rng.random(n) < 0.5).astype(np.uint8)}
    if n:
        pats["first"][0] = 1; pats["last"][-1] = 1
    return pats


def check_masks(codec, n):
    B, Q, lens, names = small_rows(n, 20, seed=n)
    for label, keep in mask_patterns(n).items():
        values = np.array([1, 0xFF, 2, 0x80], np.uint8)[np.arange(n) % 4]          # non-zero means keep
        call(codec, B, Q, lens, names, keep=np.where(keep != 0, values, 0).astype(np.uint8), row_len="x16" if n % 2 else 0)


# ---------------------------------------------------------------- test 4: both forms of the scan
def check_scan(codec, n):
    assert n in (16384, 16385, 40001)
    B, Q, lens, names = small_rows(n, 4, seed=n, name_lens=(2, 3))
    keep = (np.random.default_rng(n).random(n) < 0.5).astype(np.uint8)
    call(codec, B, Q, lens, names, keep=keep)


# ---------------------------------------------------------------- test 5: pairs and min_len
def check_pairs_and_min_len(codec):
    n = 24
    B, Q, lens, names = small_rows(n, 40, seed=5, full=True)
    keep = np.ones(n, np.uint8); start = np.zeros(n, np.int32); length = np.full(n, 40, np.int32)
    keep[0:2] = (1, 1); keep[2:4] = (1, 0); keep[4:6] = (0, 1); keep[6:8] = (0, 0)      # the four keep combinations of a pair
    min_len = 10
    length[9] = min_len - 1                                                  # R2's window one short of min_len
    length[10] = min_len - 1; length[11] = min_len                           # R1 one short, R2 exactly min_len
    length[12] = 0; keep[13] = 0                                             # short and masked mate: counted as short and mask
    r = call(codec, B, Q, lens, names, keep=keep, start=start, length=length, pairs=True, min_len=min_len)[0]
    assert (r.dropped_mask, r.dropped_short, r.dropped_mate, r.n_rows) == (5, 3, 4, 12)
    r = call(codec, B, Q, lens, names, keep=keep, start=start, length=length, pairs=False, min_len=min_len)[0]
    assert (r.dropped_mask, r.dropped_short, r.dropped_mate, r.n_rows) == (5, 3, 0, 16)
    # a window of 0: kept with min_len 0 (lens 0), dropped with min_len 1 - and the mate counted as mate
    length = np.full(n, 40, np.int32); length[3] = 0; start[3] = 40
    r, _, _, gL, _, _ = call(codec, B, Q, lens, names, start=start, length=length, pairs=True, min_len=0)
    assert r.n_rows == n and gL[3] == 0 and (r.dropped_mask, r.dropped_short, r.dropped_mate) == (0, 0, 0)
    r = call(codec, B, Q, lens, names, start=start, length=length, pairs=True, min_len=1)[0]
    assert (r.n_rows, r.dropped_mask, r.dropped_short, r.dropped_mate) == (n - 2, 0, 1, 1)


# ---------------------------------------------------------------- test 6: names
def check_name_residues(codec):
    """names of 1..40 bytes, kept and dropped so that kept names start at every residue of the output blob and lie at every residue of the input blob"""
    n = 640
    nl = [1 + (i * 7 + i // 40) % 40 for i in range(n)]
    names = [bytes(((i * 31 + k) % 94) + 33 for k in range(nl[i])) for i in range(n)]
    B, Q, lens, _ = small_rows(n, 8, seed=6)
    keep = (np.arange(n) % 3 != 1).astype(np.uint8)
    off_in = np.concatenate([[0], np.cumsum(nl)]); kept = np.nonzero(keep)[0]
    off_out = np.concatenate([[0], np.cumsum([nl[i] for i in kept])])
    assert set(nl) == set(range(1, 41)) and {int(off_in[i]) % 16 for i in kept} == set(range(16)) and {int(x) % 16 for x in off_out[:-1]} == set(range(16))
    assert off_out[-1] > 2 * 4096                                             # (several tiles of the names writer)
    for in_shift, out_shift in ((0, 0), (1, 7), (7, 15), (15, 1)):
        call(codec, B, Q, lens, names, keep=keep, in_shift=in_shift, out_shift=out_shift)
    empty = list(names)
    for i in range(100, 140):
        empty[i] = b""                                                       # names of no bytes pass through (the encoder refuses them later)
    call(codec, B, Q, lens, empty, keep=keep, out_shift=3)
    # more names start in the only tile than the writer's LDS table holds (4097): it searches the offsets themselves
    n = 6000
    B, Q, lens, _ = small_rows(n, 8, seed=9)
    sparse = [bytes(((i * 31 + k) % 94) + 33 for k in range(1 + i % 23)) if i in (0, 1500, 4200, 4300, 5999) else b"" for i in range(n)]
    keep = np.ones(n, np.uint8); keep[7] = 0
    call(codec, B, Q, lens, sparse, keep=keep, out_shift=3)
    call(codec, B, Q, lens, sparse, keep=keep, in_shift=5)


def check_long_name(codec):
    n = 40
    B, Q, lens, names = small_rows(n, 8, seed=7, name_lens=(5, 17, 33))
    names[20] = bytes(33 + k % 90 for k in range(5000))                       # longer than a 4 KiB tile
    keep = np.ones(n, np.uint8); keep[3] = 0
    call(codec, B, Q, lens, names, keep=keep, out_shift=5)
    keep[20] = 0
    call(codec, B, Q, lens, names, keep=keep, in_shift=9)


def check_no_names_and_each_output_alone(codec):
    B, Q, lens, names = small_rows(300, 33, seed=8, name_lens=(4, 9, 30))
    keep = (np.arange(300) % 4 != 0).astype(np.uint8); start = (np.arange(300) % 2).astype(np.int32) * 0
    r = call(codec, B, Q, lens, None, keep=keep, start=start)[0]
    assert (r.names_len, r.max_name) == (0, 0)
    for o in "bqlno":
        call(codec, B, Q, lens, names, keep=keep, start=start, outputs=o, row_len="x16")
    from repaq_amd import RfqError
    dev = dev_sel(codec, B, Q, lens, None)
    g = W.Guarded(codec, 4096)
    try:
        for kw in (dict(out_names=g.ptr, names_cap=4096), dict(out_name_off=g.ptr, off_cap=512)):
            with R.pytest_raises(RfqError) as ei:
                codec.select_rows(*dev.args(), row_len=40, **kw)
            assert ei.value.code == -3, ei.value
    finally:
        dev.free(); g.free()


# ---------------------------------------------------------------- test 7: sizes and refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens, names = small_rows(70, 20, seed=9)
    call(codec, B, Q, lens, names, keep=(np.arange(70) % 5 != 2).astype(np.uint8), start=np.minimum(lens - 1, 2).astype(np.int32), pairs=True)


def check_short_caps(codec):
    from repaq_amd import RfqError
    B, Q, lens, names = small_rows(200, 37, seed=10, name_lens=(3, 11, 26))
    keep = (np.arange(200) % 7 != 3).astype(np.uint8)
    e = expected(B, Q, lens, names, keep)
    n, nl, L = len(e["idx"]), e["names_len"], e["max_len"]
    assert L == 37
    dev = dev_sel(codec, B, Q, lens, names, keep)
    g = dict(b=W.Guarded(codec, n * L), q=W.Guarded(codec, n * L), l=W.Guarded(codec, 4 * n), n=W.Guarded(codec, nl), o=W.Guarded(codec, 8 * (n + 1)))
    try:
        caps = dict(bases_cap=n * L, quals_cap=n * L, lens_cap=n, names_cap=nl, off_cap=n + 1)
        ptrs = dict(out_bases=g["b"].ptr, out_quals=g["q"].ptr, out_lens=g["l"].ptr, out_names=g["n"].ptr, out_name_off=g["o"].ptr)
        before = {k: v.body() for k, v in g.items()}
        for short in list(caps) + ["row_len"]:
            kw = dict(caps, row_len=L); kw[short] -= 1
            with R.pytest_raises(RfqError) as ei:
                codec.select_rows(*dev.args(), **sel_of(dev), **ptrs, **kw)
            assert ei.value.code == -8 and "need" in ei.value.message, (short, ei.value)
            assert all(v.body() == before[k] and v.guards_intact() for k, v in g.items()), short
            _good(codec)
        r = codec.select_rows(*dev.args(), **sel_of(dev), **ptrs, row_len=L, **caps)
        assert r.n_rows == n and g["n"].body() == b"".join(e["names"]) and all(v.guards_intact() for v in g.values())
    finally:
        dev.free()
        for v in g.values():
            v.free()


def _device_refusals():
    """(label, row the message must name, mutation of (lens, start, length, name_off) in place) - start / length None: the pointer is NULL"""
    I32 = 0x7FFFFFFF

    def f(**kw):
        return kw
    return [("start_minus_1", 17, f(start={17: -1})),
            ("start_lens_plus_1_len_null", 23, f(start={23: "lens+1"}, length=None)),
            ("start_plus_len_lens_plus_1", 5, f(start={5: 3}, length={5: "lens-2"})),
            ("start_and_len_int_max", 31, f(start={31: I32}, length={31: I32})),
            ("len_minus_1", 2, f(length={2: -1})),
            ("lens_row_len_plus_1", 44, f(lens={44: "L+1"})),
            ("lens_minus_1", 0, f(lens={0: -1})),
            ("name_offsets_decrease", 12, f(name_off="swap")),
            ("last_offset_past_names_len", 59, f(name_off="past")),
            ("masked_row_is_judged_too", 8, f(start={8: -5}, keep={8: 0}))]


DEVICE_REFUSALS = _device_refusals()
DEVICE_REFUSAL_IDS = [r[0] for r in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    _, row, m = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    n, L = 60, 24
    B, Q, lens, names = small_rows(n, L, seed=11, name_lens=(2, 5, 9))
    lens = np.maximum(lens, 4).astype(np.int32)
    start = np.ones(n, np.int32); length = (lens - 2).astype(np.int32); keep = np.ones(n, np.uint8)
    val = {"lens+1": lambda i: int(lens[i]) + 1, "lens-2": lambda i: int(lens[i]) - 2, "L+1": lambda i: L + 1}
    for arr, key in ((lens, "lens"), (start, "start"), (length, "length"), (keep, "keep")):
        for i, v in (m.get(key) or {}).items():
            arr[i] = val[v](i) if isinstance(v, str) else v
    name_off = None; nl_delta = 0
    if m.get("name_off") == "swap":
        name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64); name_off[[12, 13]] = name_off[[13, 12]]
    if m.get("name_off") == "past":
        nl_delta = -1
    dev = dev_sel(codec, B, Q, lens, names, keep, start, None if ("length" in m and m["length"] is None) else length, name_off=name_off)
    g = [W.Guarded(codec, n * L), W.Guarded(codec, n * L), W.Guarded(codec, 4 * n), W.Guarded(codec, dev.names_len), W.Guarded(codec, 8 * (n + 1))]
    try:
        args = list(dev.args()); args[6] += nl_delta
        before = [x.body() for x in g]
        for query in (True, False):
            out = {} if query else dict(row_len=L, out_bases=g[0].ptr, bases_cap=n * L, out_quals=g[1].ptr, quals_cap=n * L, out_lens=g[2].ptr, lens_cap=n,
                                        out_names=g[3].ptr, names_cap=dev.names_len, out_name_off=g[4].ptr, off_cap=n + 1)
            with R.pytest_raises(RfqError) as ei:
                codec.select_rows(*args, **sel_of(dev), **out)
            assert ei.value.code == -3 and "first such row: %d)" % row in ei.value.message, (label, ei.value)
            assert [x.body() for x in g] == before and all(x.guards_intact() for x in g)
        _good(codec)
    finally:
        dev.free()
        for x in g:
            x.free()


def check_host_refusals(codec):
    from repaq_amd import RfqError
    n, L = 40, 16
    B, Q, lens, names = small_rows(n, L, seed=12)
    dev = dev_sel(codec, B, Q, lens, names, start=np.zeros(n, np.int32), length=lens)
    odd = dev_sel(codec, B[:39], Q[:39], lens[:39], names[:39])
    buf = codec.dev_put(b"\0" * (1 << 16)); b = buf.value
    try:
        full = dict(row_len=L, out_bases=C.c_void_p(b), bases_cap=n * L)

        def at(p, k):
            return C.c_void_p(p.value + k)
        calls = (("odd rows with pairs", lambda: codec.select_rows(*odd.args(), pairs=True)),
                 ("row_len 0", lambda: codec.select_rows(*dev.args(), row_len=0, out_bases=C.c_void_p(b), bases_cap=1 << 16)),
                 ("misaligned out d_lens", lambda: codec.select_rows(*dev.args(), row_len=L, out_lens=C.c_void_p(b + 2), lens_cap=1000)),
                 ("misaligned out d_name_off", lambda: codec.select_rows(*dev.args(), row_len=L, out_name_off=C.c_void_p(b + 4), off_cap=1000)),
                 ("misaligned in d_lens", lambda: codec.select_rows(n, L, dev.bases, dev.quals, at(dev.lens, 2), dev.names, dev.names_len, dev.name_off)),
                 ("misaligned in d_name_off", lambda: codec.select_rows(n, L, dev.bases, dev.quals, dev.lens, dev.names, dev.names_len, at(dev.name_off, 4))),
                 ("misaligned d_start", lambda: codec.select_rows(*dev.args(), d_start=at(dev.start, 1))),
                 ("misaligned d_len", lambda: codec.select_rows(*dev.args(), d_len=at(dev.length, 2))),
                 ("bases out on bases in", lambda: codec.select_rows(*dev.args(), row_len=L, out_bases=dev.bases, bases_cap=n * L)),
                 ("quals out ends in quals in", lambda: codec.select_rows(*dev.args(), row_len=L, out_quals=C.c_void_p(dev.quals.value - n * L + 1), quals_cap=n * L)),
                 ("lens out on lens in", lambda: codec.select_rows(*dev.args(), row_len=L, out_lens=dev.lens, lens_cap=n)),
                 ("names out inside names in", lambda: codec.select_rows(*dev.args(), row_len=L, out_names=at(dev.names, 5), names_cap=dev.names_len)),
                 ("offsets out on d_start", lambda: codec.select_rows(*dev.args(), d_start=dev.start, row_len=L, out_name_off=dev.start, off_cap=n + 1)),
                 ("bases out on the last offset in", lambda: codec.select_rows(*dev.args(), row_len=L, out_bases=at(dev.name_off, 8 * n + 7), bases_cap=n * L)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3, (what, ei.value)
            _good(codec)
        # (and a buffer of the caller's own that lies on nothing is taken)
        r = codec.select_rows(*dev.args(), **full)
        assert r.n_rows == n
    finally:
        dev.free(); odd.free(); codec.dev_free(buf)


# ---------------------------------------------------------------- tests 8 and 9: closing the square, twice
def square_selection(label, lens):
    """a seeded mask (about 80 % of the units; the first unit always) and windows that trim 0..3 bases off each end where the read has them"""
    _, _, _, paired, _ = R.BY_LABEL[label]
    n = len(lens); pe = paired != O.SE
    rng = np.random.default_rng(len(label) * 1000 + n)
    if pe:
        n -= n % 2
    units = n // 2 if pe else n
    ku = rng.random(units) < 0.8
    if units:
        ku[0] = True
    keep = np.repeat(ku, 2) if pe else ku
    keep = np.concatenate([keep, np.zeros(len(lens) - n, bool)]).astype(np.uint8)
    lens = np.asarray(lens, np.int64)
    a = np.minimum(rng.integers(0, 4, len(lens)), np.maximum(lens - 1, 0)); b = np.minimum(rng.integers(0, 4, len(lens)), np.maximum(lens - 1 - a, 0))
    return keep, a.astype(np.int32), (lens - a - b).astype(np.int32), pe


def check_square(codec, label, twice=False):
    _, fq1, fq2, paired, cb = R.BY_LABEL[label]
    recs = T.expect(fq1, fq2, paired, cb)[1]
    _, B, Q, lens, names = T.call(codec, fq1, fq2, paired, recs, extra="x16", qual_offset=33)
    keep, start, length, pe = square_selection(label, lens)
    nrows = len(lens) - (len(lens) % 2 if pe else 0)
    rows = (B[:nrows], Q[:nrows], lens[:nrows], names[:nrows])
    sel = dict(keep=keep[:nrows], start=start[:nrows], length=length[:nrows], pairs=pe, row_len="x16", out_shift=0)
    r, gB, gQ, gL, gN, raw = call(codec, *rows, **sel)
    if twice:
        assert call(codec, *rows, **sel)[5] == raw, "the same call on the same context wrote other bytes"
        return
    # the text filtered and trimmed on the host, line by line
    two = paired == O.PE_TWO_FILES
    out = [[], []]
    for i in range(nrows):
        if keep[i] and (not pe or keep[i ^ 1]):
            name, s, q = recs[i]; a, w = int(start[i]), int(length[i])
            out[i & 1 if two else 0].append(name + b"\n" + s[a:a + w] + b"\n+\n" + q[a:a + w] + b"\n")
    w1, w2 = b"".join(out[0]), b"".join(out[1])
    assert r.n_rows == len(out[0]) + len(out[1]) > 0
    got = codec.rows_to_text_bytes(gB, gQ, gL, gN, paired=paired)
    assert got == ((w1, w2) if two else w1)
    codec.clearHeader()
    img = codec.encode_rows_bytes(gB, gQ, gL, gN, paired=paired, chunk_bases=cb, **E.nolb_args(w1, w2, paired))
    assert img == O.encode_file(w1, w2, paired, cb), (label, len(img))
