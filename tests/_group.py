"""Shared helpers of the rfq_group_rows tests (tests/test_emu_group.py on the SIMT interpreter, tests/test_gpu_group.py on the MI355X).

Two oracles, both on every shape.  (a) expected(): a plain numpy / Python model written from include/rfq_hip.h - who stays by select's rule and the bin rule, a
stable sort of the kept units by bin (Python's sorted over (bin, unit)), then the rows' own bytes.  (b) per bin b, rfq_select_rows of the SAME library with the mask
keep AND bin == b spread to the rows of a unit (_select.call, which compares it with its own model): the bin's slice of the grouped output equals it byte for
byte - rows, lengths, names and the name offsets less the first.  Rows carry random bytes and every name is distinct, so a wrong order cannot pass; every
output goes into a _rows.Guarded buffer of exactly the reported size, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R
import _select as S

GR_TILE = 2048                                                               # enc/rows_group.h: elements of a workgroup of the sort
MAX_BINS = 65536
PAD_B, PAD_Q = S.PAD_B, S.PAD_Q
E_ARG, E_NOSPACE = -3, -8
FIELDS = ("n_rows", "n_bases", "names_len", "max_len", "max_name", "n_in", "dropped_mask", "dropped_short", "dropped_mate", "dropped_bin", "n_bins_used")


# ---------------------------------------------------------------- the model
def expected(B, Q, lens, names, bins, n_bins, rest=True, keep=None, start=None, length=None, pairs=False, min_len=1):
    n = len(lens); nr = 2 if pairs else 1; U = n // nr
    lens = np.asarray(lens, np.int64)
    st = np.zeros(n, np.int64) if start is None else np.asarray(start, np.int64)
    ln = lens - st if length is None else np.asarray(length, np.int64)
    k = np.ones(n, bool) if keep is None else (np.asarray(keep, np.uint8) != 0)
    binu = np.asarray(bins, np.int64).reshape(-1)
    assert len(binu) == U and (binu < n_bins).all()
    falls = np.repeat((binu < 0) & (not rest), nr)
    short = ln < min_len
    stand = k & ~falls & ~short
    kept = stand & stand.reshape(-1, 2)[:, ::-1].reshape(-1) if pairs else stand
    key = np.where(binu < 0, n_bins, binu)
    units = sorted((int(key[u]), u) for u in range(U) if kept[nr * u])        # stable: by (bin, unit)
    idx = np.array([nr * u + r for _, u in units for r in range(nr)], np.int64)
    T = n_bins + (1 if rest else 0)
    skeys = np.array([b for b, _ in units], np.int64)
    e = dict(idx=idx, n_in=n, mask=int((~k).sum()), bin=int((k & falls).sum()), short=int((k & ~falls & short).sum()), mate=int((stand & ~kept).sum()),
             lens=ln[idx].astype(np.int32), bases=[bytes(B[i, st[i]:st[i] + ln[i]]) for i in idx], quals=[bytes(Q[i, st[i]:st[i] + ln[i]]) for i in idx],
             names=None if names is None else [names[i] for i in idx], T=T, key=key, kept=kept,
             bin_off=(np.searchsorted(skeys, np.arange(T + 1), side="left") * nr).astype(np.uint64), used=len(set(skeys.tolist())))
    e["max_len"] = int(e["lens"].max()) if len(idx) else 0
    e["n_bases"] = int(e["lens"].sum())
    e["names_len"] = sum(map(len, e["names"])) if names is not None else 0
    e["max_name"] = max(map(len, e["names"])) if names is not None and len(idx) else 0
    assert n == len(idx) + e["mask"] + e["bin"] + e["short"] + e["mate"] and int(e["bin_off"][T]) == len(idx)
    if pairs:
        assert (idx[0::2] % 2 == 0).all() and (idx[1::2] == idx[0::2] + 1).all()   # R1 first, R2 next to it
    return e


def fields_of(r):
    return tuple(int(getattr(r, f)) for f in FIELDS)


def fields_want(e):
    return (len(e["idx"]), e["n_bases"], e["names_len"], e["max_len"], e["max_name"], e["n_in"], e["mask"], e["short"], e["mate"], e["bin"], e["used"])


def case_rows(n, L, seed, names=True, min_row=1):
    """n rows of stride L with random bytes in and behind the reads, lengths min_row .. L, names "@<seed>.<row>" + a tail of 0 .. 6 bytes: every one distinct"""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, (n, L), dtype=np.uint8); Q = rng.integers(0, 256, (n, L), dtype=np.uint8)
    lens = rng.integers(min_row, L + 1, n).astype(np.int32)
    nm = [b"@%d.%d" % (seed, i) + b"abcdef"[:i % 7] for i in range(n)] if names else None
    return B, Q, lens, nm


def dev_group(codec, B, Q, lens, names, bins, keep=None, start=None, length=None, shift=0, name_off=None):
    return W.DevRows(codec, B, Q, lens, names, shift=shift, name_off=name_off, keep=(keep, np.uint8), start=(start, np.int32), length=(length, np.int32),
                     bin=(np.asarray(bins, np.int32), np.int32))


def kw_of(dev, n_bins, rest, pairs, min_len):
    return dict(d_bin=dev.bin, n_bins=n_bins, rest=rest, pairs=pairs, min_len=min_len, d_keep=dev.keep, d_start=dev.start, d_len=dev.length)


def _split_raw(raw, outputs):
    """compact_into_guarded's raw bodies by letter"""
    return dict(zip([o for o in "bqlno" if o in outputs], raw))


def call(codec, B, Q, lens, names, bins, n_bins, rest=True, keep=None, start=None, length=None, pairs=False, min_len=1, row_len=None, in_shift=0, out_shift=0,
         outputs="bqlnog", per_bin=True):
    """A size query and one rfq_group_rows into Guarded buffers of exactly the reported sizes, compared with the model (a) and, per bin that holds a row, with
    rfq_select_rows of the same library (b).  outputs: b q l n o as _rows.compact_into_guarded, g = d_bin_off.  Returns (model, result, raw bytes of every output)."""
    e = expected(B, Q, lens, names, bins, n_bins, rest, keep, start, length, pairs, min_len)
    T = e["T"]
    if names is None:
        outputs = outputs.replace("n", "").replace("o", "")
    five = outputs.replace("g", "")
    dev = dev_group(codec, B, Q, lens, names, bins, keep, start, length, shift=in_shift)
    gbo = W.Guarded(codec, 8 * (T + 1)) if "g" in outputs else None
    try:
        kw = kw_of(dev, n_bins, rest, pairs, min_len)
        q = codec.group_rows(*dev.args(), **kw)
        assert fields_of(q) == fields_want(e), dict(zip(FIELDS, zip(fields_of(q), fields_want(e))))
        assert q.n_in == q.n_rows + q.dropped_mask + q.dropped_bin + q.dropped_short + q.dropped_mate
        L = S.out_len(e["max_len"], row_len)
        n = len(e["idx"])

        def rows_differ(kind, g, wantr, bad):
            return "%s rows differ: %d of %d, first %d (input row %d): %r / %r" % (kind, len(bad), n, bad[0], e["idx"][bad[0]], bytes(g[bad[0]][:48]), bytes(wantr[bad[0]][:48]))
        bo = dict(out_bin_off=gbo.ptr, bin_cap=T + 1) if gbo else {}
        r, gB, gQ, gL, raw = W.compact_into_guarded(codec, lambda **out: codec.group_rows(*dev.args(), **out, **bo, **kw), e, L, PAD_B, PAD_Q, five, out_shift,
                                                    rows_differ=rows_differ)
        assert fields_of(r) == fields_of(q), "the size query and the writing call report different results"
        got = _split_raw(raw, five)
        if gbo:
            assert gbo.guards_intact(), "a guard around d_bin_off was written"
            got["g"] = gbo.body()
            off = np.frombuffer(got["g"], np.uint64)
            assert np.array_equal(off, e["bin_off"]), ("bin_off differs", off[:8], e["bin_off"][:8])
            assert int(off[T]) == r.n_rows
    finally:
        dev.free()
        if gbo:
            gbo.free()
    if per_bin:
        check_per_bin(codec, B, Q, lens, names, e, got, L, n_bins, keep, start, length, pairs, min_len)
    return e, r, got


def check_per_bin(codec, B, Q, lens, names, e, got, L, n_bins, keep, start, length, pairs, min_len):
    """oracle (b): every bin's slice equals rfq_select_rows under the mask keep AND bin == b"""
    nr = 2 if pairs else 1
    k = np.ones(len(lens), np.uint8) if keep is None else (np.asarray(keep, np.uint8) != 0).astype(np.uint8)
    off = e["bin_off"].astype(np.int64)
    noff = np.frombuffer(got["o"], np.uint64).astype(np.int64) if "o" in got else None
    for b in range(e["T"]):
        r0, r1 = int(off[b]), int(off[b + 1])
        if r0 == r1:
            continue
        mask = (k & np.repeat(e["key"] == b, nr)).astype(np.uint8)
        rule = L if L > 1 else None
        _, sB, sQ, sL, sN, sraw = S.call(codec, B, Q, lens, names, keep=mask, start=start, length=length, pairs=pairs, min_len=min_len, row_len=rule,
                                         outputs="".join(o for o in "bqlno" if o in got))
        sel = _split_raw(sraw, [o for o in "bqlno" if o in got])
        for o, width in (("b", L), ("q", L), ("l", 4)):
            if o in got:
                assert sel[o] == got[o][r0 * width:r1 * width], "bin %d: output %s differs from select_rows under the bin's mask" % (b, o)
        if noff is not None:
            so = np.frombuffer(sel["o"], np.uint64).astype(np.int64)
            assert np.array_equal(so, noff[r0:r1 + 1] - noff[r0]), "bin %d: the name offsets less the first differ from select_rows'" % b
            if "n" in got:
                assert sel["n"] == got["n"][int(noff[r0]):int(noff[r1])], "bin %d: the names differ from select_rows'" % b


# ---------------------------------------------------------------- test 1: unit counts around a wave, a workgroup's step and a tile
UNITS = (0, 1, 63, 64, 65, 255, 256, 257, GR_TILE - 1, GR_TILE, GR_TILE + 1, 2 * GR_TILE + 1)


def check_units(codec, U):
    """U units, as rows and as pairs, over three bins and the rest bin in a seeded order, part of them masked; the stride of 9 keeps rows of 1 .. 9 bytes"""
    for pairs in (False, True):
        n = (2 if pairs else 1) * U
        rng = np.random.default_rng(7000 + U)
        B, Q, lens, names = case_rows(n, 9, 100 + U)
        bins = rng.integers(-1, 3, U).astype(np.int32)
        keep = (rng.random(n) < 0.9).astype(np.uint8)
        e, r, _ = call(codec, B, Q, lens, names, bins, 3, keep=keep, pairs=pairs, row_len="x16" if U % 2 else None)
        assert U < 63 or (r.n_bins_used == 4 and r.dropped_mask > 0)


def check_many_units(codec, U=40_003):
    """more units than a few tiles: 20 tiles of the sort, several tiles of the scans; the grid is not capped, so this is the count at which every launch of the
    call has many workgroups and a part-empty last one"""
    rng = np.random.default_rng(7100)
    B, Q, lens, names = case_rows(U, 4, 7100)
    bins = rng.integers(-1, 300, U).astype(np.int32)
    e, r, _ = call(codec, B, Q, lens, names, bins, 300, per_bin=False)
    assert r.n_bins_used == 301 and r.n_rows == U


# ---------------------------------------------------------------- test 2: total bins around the one-pass / two-pass seam and at the limits
TOTALS = (1, 2, 255, 256, 257, 4097, MAX_BINS)


def check_totals(codec, T):
    """T bins in all, with and without the rest bin: about 300 units spread over the first, the last and a few dozen other bins (most bins are empty beyond 257)"""
    rng = np.random.default_rng(7200 + T)
    U = 300
    B, Q, lens, names = case_rows(U, 12, 200 + T % 1000)
    for rest in (True, False):
        n_bins = T - 1 if rest else T
        if n_bins < 1:
            continue
        some = np.unique(np.concatenate([[0, n_bins - 1, n_bins // 2], rng.integers(0, n_bins, 30)]))
        bins = some[rng.integers(0, len(some), U)].astype(np.int32)
        bins[:4] = (n_bins - 1, 0, n_bins - 1, 0)
        bins[rng.random(U) < 0.1] = -1
        bins[7] = -1; bins[8] = -0x80000000
        e, r, _ = call(codec, B, Q, lens, names, bins, n_bins, rest=rest)
        assert (r.dropped_bin > 0) == (not rest) and e["T"] == T


# ---------------------------------------------------------------- test 3: bin patterns
def patterns(U, n_bins):
    u = np.arange(U)
    p = {"one_bin": np.full(U, n_bins // 2), "own_bin": u.copy(), "descending": U - 1 - u, "sorted": (u * n_bins) // max(U, 1), "round_robin": u % 5,
         "empty_first_mid_last": np.where(u % 2 == 0, 2, n_bins - 3), "high_byte_only": (u % 3) << 8, "low_byte_only": 0x300 + u % 7}
    return {k: v.astype(np.int32) for k, v in p.items()}


PATTERN_IDS = tuple(patterns(10, 1024))


def check_pattern(codec, label):
    """U = 130 units (three waves, the last of two lanes; bins with more units than a wave and bins of one unit) over 1024 bins (two passes) and, where the pattern fits, over 256 (one pass)"""
    U = 130
    B, Q, lens, names = case_rows(U, 10, 300 + PATTERN_IDS.index(label))
    for n_bins in (1024, 256):
        bins = patterns(U, n_bins)[label]
        if int(bins.max()) >= n_bins:
            assert n_bins == 256 and label in ("high_byte_only", "low_byte_only")
            continue
        e, r, _ = call(codec, B, Q, lens, names, bins, n_bins, rest=(n_bins == 1024))
        assert r.n_rows == U
        if label == "descending":
            assert (e["idx"] == np.arange(U)[::-1]).all()                    # every row moves
        if label == "sorted":
            assert (e["idx"] == np.arange(U)).all()


# ---------------------------------------------------------------- test 4: the rest bin
def check_rest(codec):
    U = 90
    B, Q, lens, names = case_rows(U, 8, 41)
    for negatives in (True, False):
        bins = (np.arange(U) % 4).astype(np.int32)
        if negatives:
            bins[::5] = -1; bins[3] = -7
        for rest in (True, False):
            e, r, got = call(codec, B, Q, lens, names, bins, 4, rest=rest)
            want_bin = int((bins < 0).sum()) if not rest else 0
            assert r.dropped_bin == want_bin and r.n_rows == U - want_bin
            off = np.frombuffer(got["g"], np.uint64)
            assert len(off) == 4 + rest + 1 and int(off[-1]) == r.n_rows
            assert not rest or int(off[5] - off[4]) == int((bins < 0).sum())


# ---------------------------------------------------------------- test 5: pairs
def check_pairs(codec):
    """pairs whose mate falls to the mask and to min_len - `start` eats a read, as demux_rows leaves it -, with the reasons counted in their order"""
    U = 70; n = 2 * U
    B, Q, lens, names = case_rows(n, 24, 51, min_row=6)
    bins = (np.arange(U) % 3 - 1).astype(np.int32)                           # -1, 0, 1 in turn
    keep = np.ones(n, np.uint8); start = np.full(n, 3, np.int32)
    keep[10] = 0                                                             # R1 masked: R2 falls as mate
    keep[17] = 0                                                             # R2 masked
    start[24] = lens[24]                                                     # the barcode used up R1: short, R2 falls as mate
    start[31] = lens[31]                                                     # ... R2
    keep[40] = 0; start[41] = lens[41]                                       # masked and short in one pair: counted as mask and short
    e, r, _ = call(codec, B, Q, lens, names, bins, 2, rest=True, keep=keep, start=start, pairs=True)
    assert (r.dropped_mask, r.dropped_bin, r.dropped_short, r.dropped_mate, r.n_rows) == (3, 0, 3, 4, n - 10)
    # rest = 0: the units of bin -1 fall, counted in front of `short` and behind the mask (units 0, 3, .. 69: rows 24 / 25 are unit 12's)
    e, r, _ = call(codec, B, Q, lens, names, bins, 2, rest=False, keep=keep, start=start, pairs=True)
    fall = np.repeat(bins < 0, 2)
    assert r.dropped_bin == int((fall & (keep != 0)).sum()) and r.dropped_mask == 3 and r.n_rows == len(e["idx"]) > 0
    assert r.dropped_short == int(((start == lens) & ~fall & (keep != 0)).sum())
    # min_len 0 keeps the empty read
    e, r, _ = call(codec, B, Q, lens, names, bins, 2, keep=keep, start=start, pairs=True, min_len=0)
    assert r.dropped_short == 0 and r.dropped_mate == 3


# ---------------------------------------------------------------- test 6: names
def check_names(codec):
    U = 150
    B, Q, lens, names = case_rows(U, 7, 61)
    bins = (np.arange(U) * 7 % 5).astype(np.int32)
    e, r, _ = call(codec, B, Q, lens, None, bins, 5)                          # rows without names
    assert (r.names_len, r.max_name) == (0, 0)
    names[3] = b""; names[77] = b""                                          # names of no bytes
    names[40] = b"@long." + bytes(33 + k % 90 for k in range(5000))          # longer than 255 bytes, and than a tile of the names writer
    e, r, _ = call(codec, B, Q, lens, names, bins, 5, out_shift=3)
    assert r.max_name == len(names[40]) and r.names_len == sum(map(len, names))
    keep = np.ones(U, np.uint8); keep[40] = 0
    call(codec, B, Q, lens, names, bins, 5, keep=keep, in_shift=9)
    from repaq_amd import RfqError
    dev = dev_group(codec, B, Q, lens, None, bins)
    g = W.Guarded(codec, 4096)
    try:
        for kw in (dict(out_names=g.ptr, names_cap=4096), dict(out_name_off=g.ptr, off_cap=512)):
            with R.pytest_raises(RfqError) as ei:
                codec.group_rows(*dev.args(), d_bin=dev.bin, n_bins=5, row_len=8, **kw)
            assert ei.value.code == E_ARG, ei.value
    finally:
        dev.free(); g.free()


# ---------------------------------------------------------------- test 7: layout, no rows left, partial outputs, determinism
def check_layout(codec):
    """unaligned row buffers and strides that are no multiple of 16, in and out; both aligned; windows that start inside a group"""
    for L, rule, in_shift, out_shift in ((37, 1, 5, 3), (48, "x16", 0, 0)):
        U = 120
        B, Q, lens, names = case_rows(U, L, 70 + L)
        bins = (np.arange(U) % 4 - 1).astype(np.int32)
        start = (np.arange(U) % 3).astype(np.int32); start = np.minimum(start, lens - 1).astype(np.int32)
        call(codec, B, Q, lens, names, bins, 3, start=start, row_len=rule, in_shift=in_shift, out_shift=out_shift)


def check_nothing_kept(codec):
    U = 66
    B, Q, lens, names = case_rows(U, 8, 81)
    bins = (np.arange(U) % 3).astype(np.int32)
    e, r, got = call(codec, B, Q, lens, names, bins, 3, keep=np.zeros(U, np.uint8))
    assert r.n_rows == 0 and got["o"] == b"\0" * 8 and got["g"] == b"\0" * 40 and r.n_bins_used == 0
    e, r, got = call(codec, B, Q, lens, names, np.full(U, -1, np.int32), 3, rest=False)
    assert r.n_rows == 0 and r.dropped_bin == U


def check_partial_outputs(codec):
    U = 300
    B, Q, lens, names = case_rows(U, 20, 91)
    bins = (np.arange(U) * 13 % 11 - 1).astype(np.int32)
    keep = (np.arange(U) % 6 != 1).astype(np.uint8)
    full = call(codec, B, Q, lens, names, bins, 10, keep=keep)[2]
    for outputs in ("g", "l", "bqlg", "no", "b"):
        got = call(codec, B, Q, lens, names, bins, 10, keep=keep, outputs=outputs, per_bin=False)[2]
        assert set(got) == set(outputs) and all(got[o] == full[o] for o in outputs), outputs
    # d_bin_off alone wants no row_len: the rows per bin without moving a row
    dev = dev_group(codec, B, Q, lens, names, bins, keep)
    g = W.Guarded(codec, 8 * 12)
    try:
        r = codec.group_rows(*dev.args(), d_bin=dev.bin, n_bins=10, d_keep=dev.keep, out_bin_off=g.ptr, bin_cap=12)
        assert g.guards_intact() and g.body() == full["g"] and r.n_rows == int(np.frombuffer(full["g"], np.uint64)[-1])
    finally:
        dev.free(); g.free()


def check_same_bytes_twice(codec):
    U = 2 * GR_TILE + 77
    rng = np.random.default_rng(101)
    B, Q, lens, names = case_rows(U, 6, 101)
    bins = rng.integers(-1, 700, U).astype(np.int32)
    a = call(codec, B, Q, lens, names, bins, 700, per_bin=False)[2]
    b = call(codec, B, Q, lens, names, bins, 700, per_bin=False)[2]
    assert set(a) == set("bqlnog") and a == b, "the same call on the same context wrote other bytes"


# ---------------------------------------------------------------- test 8: refusals
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens, names = case_rows(70, 12, 9)
    bins = (np.arange(35) % 4 - 1).astype(np.int32)
    call(codec, B, Q, lens, names, bins, 3, keep=(np.arange(70) % 9 != 2).astype(np.uint8), start=np.minimum(lens - 1, 2).astype(np.int32), pairs=True)


def check_host_refusals(codec):
    from repaq_amd import RfqError
    n, L = 40, 16
    B, Q, lens, names = case_rows(n, L, 12)
    bins = (np.arange(n) % 3).astype(np.int32)
    dev = dev_group(codec, B, Q, lens, names, bins, keep=np.ones(n, np.uint8), start=np.zeros(n, np.int32), length=lens)
    odd = dev_group(codec, B[:39], Q[:39], lens[:39], names[:39], bins[:39])
    buf = codec.dev_put(b"\0" * (1 << 16)); b = buf.value
    try:
        def at(p, k):
            return C.c_void_p(p.value + k)

        def G(*rows, **kw):
            kw.setdefault("d_bin", dev.bin); kw.setdefault("n_bins", 3)
            return codec.group_rows(*(rows or dev.args()), **kw)
        out = dict(row_len=L, out_bases=C.c_void_p(b), bases_cap=n * L)
        calls = (("rows in pairs", lambda: G(*odd.args(), d_bin=odd.bin, pairs=True)),
                 ("pairs must be 0 or 1", lambda: G(raw=dict(pairs=2))),
                 ("row_len must be >= 1", lambda: G(row_len=0, out_bases=C.c_void_p(b), bases_cap=1 << 16)),
                 ("null d_bin", lambda: G(d_bin=None)),
                 ("n_bins must be >= 1", lambda: G(n_bins=0)),
                 ("n_bins + rest is at most 65536", lambda: G(n_bins=65536, rest=True)),
                 ("n_bins + rest is at most 65536", lambda: G(n_bins=0xFFFFFFFF, rest=True)),
                 ("n_bins + rest is at most 65536", lambda: G(n_bins=65537, rest=False)),
                 ("rest must be 0 or 1", lambda: G(raw=dict(rest=2))),
                 ("rest must be 0 or 1", lambda: G(raw=dict(rest=-1))),
                 ("4-byte aligned", lambda: G(d_bin=at(dev.bin, 2))),
                 ("4-byte aligned", lambda: G(row_len=L, out_lens=C.c_void_p(b + 2), lens_cap=1000)),
                 ("4-byte aligned", lambda: G(n, L, dev.bases, dev.quals, at(dev.lens, 2), dev.names, dev.names_len, dev.name_off)),
                 ("4-byte aligned", lambda: G(d_start=at(dev.start, 1))),
                 ("4-byte aligned", lambda: G(d_len=at(dev.length, 2))),
                 ("d_name_off must be 8-byte aligned", lambda: G(row_len=L, out_name_off=C.c_void_p(b + 4), off_cap=1000)),
                 ("d_name_off must be 8-byte aligned", lambda: G(n, L, dev.bases, dev.quals, dev.lens, dev.names, dev.names_len, at(dev.name_off, 4))),
                 ("d_bin_off must be 8-byte aligned", lambda: G(out_bin_off=C.c_void_p(b + 4), bin_cap=5)),
                 ("d_bases overlaps the input rows->d_bases", lambda: G(row_len=L, out_bases=dev.bases, bases_cap=n * L)),
                 ("d_quals overlaps the input", lambda: G(row_len=L, out_quals=C.c_void_p(dev.quals.value - n * L + 1), quals_cap=n * L)),
                 ("d_lens overlaps the input rows->d_lens", lambda: G(row_len=L, out_lens=dev.lens, lens_cap=n)),
                 ("d_names overlaps the input rows->d_names", lambda: G(row_len=L, out_names=at(dev.names, 5), names_cap=dev.names_len)),
                 ("d_name_off overlaps the input", lambda: G(d_start=dev.start, row_len=L, out_name_off=dev.start, off_cap=n + 1)),
                 ("d_lens overlaps the input d_bin", lambda: G(row_len=L, out_lens=dev.bin, lens_cap=n)),
                 ("d_bases overlaps the input", lambda: G(row_len=L, out_bases=at(dev.bin, 4 * n - 1), bases_cap=n * L)),
                 ("d_bin_off overlaps the input d_bin", lambda: G(out_bin_off=at(dev.bin, 8 - dev.bin.value % 8), bin_cap=4)),
                 ("d_bin_off overlaps the input rows->d_lens", lambda: G(out_bin_off=at(dev.lens, 8 - dev.lens.value % 8), bin_cap=4)),
                 ("d_bin_off overlaps the input d_keep", lambda: G(d_keep=dev.keep, out_bin_off=at(dev.keep, 8 - dev.keep.value % 8), bin_cap=4)),
                 ("too many rows", lambda: G(0xFFFFFFF0, 1, dev.bases, dev.quals, dev.lens)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == E_ARG and what in ei.value.message, (what, ei.value)
            _good(codec)
        # (buffers of the caller's own that lie on nothing are taken)
        r = G(**out, out_bin_off=C.c_void_p(b + 32768), bin_cap=5)
        assert r.n_rows == n
    finally:
        dev.free(); odd.free(); codec.dev_free(buf)


def check_short_caps(codec):
    """RFQ_E_NOSPACE for every cap one short, bin_cap among them: the message says "need", nothing is written"""
    from repaq_amd import RfqError
    U = 200
    B, Q, lens, names = case_rows(U, 37, 10)
    lens[5] = 37
    bins = (np.arange(U) % 6 - 1).astype(np.int32)
    keep = (np.arange(U) % 7 != 3).astype(np.uint8)
    e = expected(B, Q, lens, names, bins, 5, True, keep)
    n, nl, L, T = len(e["idx"]), e["names_len"], e["max_len"], 6
    dev = dev_group(codec, B, Q, lens, names, bins, keep)
    g = dict(b=W.Guarded(codec, n * L), q=W.Guarded(codec, n * L), l=W.Guarded(codec, 4 * n), n=W.Guarded(codec, nl), o=W.Guarded(codec, 8 * (n + 1)), g=W.Guarded(codec, 8 * (T + 1)))
    try:
        caps = dict(bases_cap=n * L, quals_cap=n * L, lens_cap=n, names_cap=nl, off_cap=n + 1, bin_cap=T + 1)
        ptrs = dict(out_bases=g["b"].ptr, out_quals=g["q"].ptr, out_lens=g["l"].ptr, out_names=g["n"].ptr, out_name_off=g["o"].ptr, out_bin_off=g["g"].ptr)
        before = {k: v.body() for k, v in g.items()}
        sel = dict(d_bin=dev.bin, n_bins=5, d_keep=dev.keep)
        for short in list(caps) + ["row_len"]:
            kw = dict(caps, row_len=L); kw[short] -= 1
            with R.pytest_raises(RfqError) as ei:
                codec.group_rows(*dev.args(), **sel, **ptrs, **kw)
            assert ei.value.code == E_NOSPACE and "need" in ei.value.message, (short, ei.value)
            assert short != "bin_cap" or "bin_cap < T + 1" in ei.value.message
            assert all(v.body() == before[k] and v.guards_intact() for k, v in g.items()), short
            _good(codec)
        r = codec.group_rows(*dev.args(), **sel, **ptrs, row_len=L, **caps)
        assert r.n_rows == n and g["n"].body() == b"".join(e["names"]) and all(v.guards_intact() for v in g.values())
        assert np.array_equal(np.frombuffer(g["g"].body(), np.uint64), e["bin_off"])
    finally:
        dev.free()
        for v in g.values():
            v.free()


DEVICE_REFUSALS = [(v, u) for v in ("n_bins", "int32_max") for u in ("first", "last", "masked")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def _refused_untouched(codec, dev, sel, n, L, T, needles):
    """a size query and a writing call are both refused with E_ARG and one of the needles; outputs pre-filled with a pattern stay untouched"""
    from repaq_amd import RfqError
    g = [W.Guarded(codec, n * L), W.Guarded(codec, n * L), W.Guarded(codec, 4 * n), W.Guarded(codec, max(dev.names_len, 1)), W.Guarded(codec, 8 * (n + 1)), W.Guarded(codec, 8 * (T + 1))]
    try:
        before = [x.body() for x in g]
        for query in (True, False):
            out = {} if query else dict(row_len=L, out_bases=g[0].ptr, bases_cap=n * L, out_quals=g[1].ptr, quals_cap=n * L, out_lens=g[2].ptr, lens_cap=n,
                                        out_names=g[3].ptr, names_cap=max(dev.names_len, 1), out_name_off=g[4].ptr, off_cap=n + 1, out_bin_off=g[5].ptr, bin_cap=T + 1)
            with R.pytest_raises(RfqError) as ei:
                codec.group_rows(*dev.args(), **sel, **out)
            assert ei.value.code == E_ARG and any(x in ei.value.message for x in needles), (needles, ei.value)
            assert [x.body() for x in g] == before and all(x.guards_intact() for x in g)
    finally:
        for x in g:
            x.free()


def check_device_refusal(codec, label):
    """bin == n_bins and bin = INT32_MAX in the first unit, the last unit and a unit `keep` masks - rows and pairs, one tile and three"""
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    n_bins = 9
    for U, pairs in ((60, False), (2 * GR_TILE + 9, False), (50, True)):
        nr = 2 if pairs else 1; n = nr * U; L = 6
        B, Q, lens, names = case_rows(n, L, 13)
        bins = (np.arange(U) % 10 - 1).astype(np.int32)
        unit = dict(first=0, last=U - 1, masked=U // 2)[where]
        bins[unit] = n_bins if value == "n_bins" else 0x7FFFFFFF
        keep = np.ones(n, np.uint8)
        if where == "masked":
            keep[nr * unit:nr * unit + nr] = 0
        dev = dev_group(codec, B, Q, lens, names, bins, keep)
        try:
            for rest in (True, False):
                _refused_untouched(codec, dev, dict(d_bin=dev.bin, n_bins=n_bins, rest=rest, pairs=pairs, d_keep=dev.keep), n, L, n_bins + rest, ["first such unit: %d)" % unit])
        finally:
            dev.free()
        _good(codec)
    # two bad units: the first is named
    bins = np.zeros(U, np.int32); bins[41] = 99; bins[7] = 9
    dev = dev_group(codec, B, Q, lens, names, bins)
    try:
        _refused_untouched(codec, dev, dict(d_bin=dev.bin, n_bins=n_bins, pairs=True), n, L, n_bins + 1, ["first such unit: 7)"])
    finally:
        dev.free()
    _good(codec)


def check_device_refusals_together(codec):
    """a bad bin with each of select's device refusals in the same call: some error is reported, nothing is written"""
    n, L = 60, 24
    for label, row, m in S.DEVICE_REFUSALS:
        B, Q, lens, names = case_rows(n, L, 11, min_row=4)
        start = np.ones(n, np.int32); length = (lens - 2).astype(np.int32); keep = np.ones(n, np.uint8)
        val = {"lens+1": lambda i: int(lens[i]) + 1, "lens-2": lambda i: int(lens[i]) - 2, "L+1": lambda i: L + 1}
        for arr, key in ((lens, "lens"), (start, "start"), (length, "length"), (keep, "keep")):
            for i, v in (m.get(key) or {}).items():
                arr[i] = val[v](i) if isinstance(v, str) else v
        name_off = None
        if m.get("name_off") == "swap":
            name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64); name_off[[12, 13]] = name_off[[13, 12]]
        if m.get("name_off") == "past":
            name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64); name_off[n] += 1
        bins = (np.arange(n) % 5).astype(np.int32); bins[33] = 5
        dev = dev_group(codec, B, Q, lens, names, bins, keep, start, None if ("length" in m and m["length"] is None) else length, name_off=name_off)
        try:
            sel = dict(d_bin=dev.bin, n_bins=5, d_keep=dev.keep, d_start=dev.start, d_len=dev.length)
            _refused_untouched(codec, dev, sel, n, L, 6, ["first such row: %d)" % row, "first such unit: 33)"])
        finally:
            dev.free()
        _good(codec)


# ---------------------------------------------------------------- test 9: state
def check_state(codec):
    """the scratch is reused at other sizes - a large call, a tiny one, a large one with another T -; select_rows, merge_rows and demux_rows give before and after
    a group call what they gave; a refused call is followed by a good one"""
    import _demux as D
    import _history as Hs
    from repaq_amd import RfqError
    rng = np.random.default_rng(900)
    U = 3 * GR_TILE + 5
    Bl, Ql, ll, nl = case_rows(U, 5, 900)
    Bs, Qs, ls, ns = case_rows(3, 5, 901)
    big_a = rng.integers(-1, 1000, U).astype(np.int32); big_b = rng.integers(-1, 40, U).astype(np.int32)
    first = call(codec, Bl, Ql, ll, nl, big_a, 1000, per_bin=False)[2]
    call(codec, Bs, Qs, ls, ns, np.array([1, 0, 1], np.int32), 2, rest=False)
    call(codec, Bl, Ql, ll, nl, big_b, 40, per_bin=False)
    call(codec, Bs, Qs, ls, ns, np.array([300, -1, 2], np.int32), 301)
    assert call(codec, Bl, Ql, ll, nl, big_a, 1000, per_bin=False)[2] == first
    calls = Hs.calls()
    for kind in ("select_rows", "merge_rows"):
        before = getattr(calls, kind)(codec)
        _good(codec)
        assert getattr(calls, kind)(codec) == before, "a group call changed what %s gives" % kind
    D._good(codec); _good(codec); D._good(codec)
    dev = dev_group(codec, Bs, Qs, ls, ns, np.array([0, 2, 0], np.int32))
    try:
        with R.pytest_raises(RfqError) as ei:
            codec.group_rows(*dev.args(), d_bin=dev.bin, n_bins=2)
        assert ei.value.code == E_ARG and "first such unit: 1)" in ei.value.message
    finally:
        dev.free()
    _good(codec)
