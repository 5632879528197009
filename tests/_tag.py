"""Shared helpers of the tests of rfq_select_rows with a tag (rfq_name_tag: UMI extraction) - tests/test_emu_tag.py on the SIMT interpreter, tests/test_gpu_tag.py
on the MI355X.

Nothing expected comes from the code under test: the model is a plain Python loop over rows that builds every expected name from the rules of include/rfq_hip.h -
part(i), the unit's tag T, the inserted text X = sep, (prefix, join), T, its place in the name -, and _select.expected() makes the kept rows from those names with
numpy.  Every output goes into a _rows.Guarded buffer of exactly the reported size, the guards are checked after each call, and every check runs on the default
formulation and on RFQ_TAG=general and compares the bytes of the two."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R
import _select as S

OPTION = "RFQ_TAG"
PATHS = (None, "general")
E_ARG, E_DATA, E_NOSPACE = -3, -5, -8
AT_SPACE, AT_END = 0, 1
RESULT = ("n_rows", "n_bases", "names_len", "max_len", "max_name", "n_in", "dropped_mask", "dropped_short", "dropped_mate")


# ---------------------------------------------------------------- the model
class Tag:
    """a tag as the model and a call take it: the two arrays and the four settings"""
    def __init__(self, start, length, sep=b":", prefix=b"", join=b"_", at=AT_SPACE):
        self.start, self.length = np.asarray(start, np.int32), np.asarray(length, np.int32)
        self.sep, self.prefix, self.join, self.at = sep, prefix, join, at


def part(B, i, ts, tl, codes):
    raw = bytes(B[i, ts:ts + tl])
    return bytes(b"ACGTN"[c] for c in raw) if codes else raw


def tagged_names(B, names, tag, pairs=False, codes=False):
    """the name of every row, kept or not, with its unit's X in its place"""
    n = len(names); out = []
    for i in range(n):
        rows = (i & ~1, (i & ~1) + 1) if pairs else (i,)
        parts = [part(B, r, int(tag.start[r]), int(tag.length[r]), codes) for r in rows]
        T = (tag.join if all(parts) else b"").join(parts) if pairs else parts[0]
        X = (tag.sep + (tag.prefix + tag.join if tag.prefix else b"") + T) if T else b""
        name = names[i]
        at = len(name)
        if tag.at == AT_SPACE and b" " in name:
            at = name.index(b" ")
        out.append(name[:at] + X + name[at:])
        assert len(X) <= 81
    return out


# ---------------------------------------------------------------- rows and calls
def dev_tag(codec, B, Q, lens, names, tag, keep=None, start=None, length=None, shift=0):
    return W.DevRows(codec, B, Q, lens, names, shift=shift, keep=(keep, np.uint8), start=(start, np.int32), length=(length, np.int32),
                     tstart=(tag.start if tag is not None else None, np.int32), tlen=(tag.length if tag is not None else None, np.int32))


def tag_of(dev, tag, raw=None):
    return None if tag is None else dict(d_tag_start=dev.tstart, d_tag_len=dev.tlen, prefix=tag.prefix, sep=tag.sep, join=tag.join, at=tag.at, raw=raw)


def result_of(r):
    return tuple(int(getattr(r, f)) for f in RESULT)


def run(codec, B, Q, lens, names, tag, keep=None, start=None, length=None, pairs=False, min_len=1, codes=False, in_shift=0, out_shift=0, outputs="bqlno", row_len="x16", what=""):
    """one size query and one rfq_select_rows with the tag (None: the plain call) into Guarded buffers of exactly the reported sizes, both against the model;
    returns (result fields, raw bytes of every output body)"""
    want = names if tag is None else tagged_names(B, names, tag, pairs, codes)
    e = S.expected(B, Q, lens, want, keep, start, length, pairs, min_len)
    dev = dev_tag(codec, B, Q, lens, names, tag, keep, start, length, shift=in_shift)
    try:
        kw = dict(pairs=pairs, min_len=min_len, codes=codes, tag=tag_of(dev, tag), **S.sel_of(dev))
        q = codec.select_rows(*dev.args(), **kw)
        wantr = (len(e["idx"]), e["n_bases"], e["names_len"], e["max_len"], e["max_name"], e["n_in"], e["mask"], e["short"], e["mate"])
        assert result_of(q) == wantr, (what, "size query", result_of(q), wantr)
        r, _, _, _, raw = W.compact_into_guarded(codec, lambda **out: codec.select_rows(*dev.args(), **out, **kw), e, S.out_len(e["max_len"], row_len), S.PAD_B, S.PAD_Q,
                                                 outputs, out_shift, what=what + " ", rows_differ=lambda kind, g, w, bad: "%s rows differ, first %d" % (kind, bad[0]))
        assert result_of(r) == wantr, (what, "the writing call", result_of(r), wantr)
        return wantr, raw
    finally:
        dev.free()


def check(codec, B, Q, lens, names, tag, paths=PATHS, what="", **kw):
    """the call equals the model on every formulation, and the formulations give equal bytes; returns the result fields"""
    try:
        got = []
        for path in paths:
            codec.set_option(OPTION, path)
            got.append(run(codec, B, Q, lens, names, tag, what="%s option %s:" % (what, path or "default"), **kw))
        assert all(g == got[0] for g in got), what + " the formulations give different bytes"
        return got[0][0]
    finally:
        codec.set_option(OPTION, None)


def rows(n, L, seed, codes=False, full=True, letters=b"ACGTNacgtn"):
    """n rows of stride L: bases as codes 0 .. 4 or as letters (lower case and N among them), random quality bytes, lengths L (full) or 1 .. L"""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 5, (n, L)).astype(np.uint8) if codes else np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), (n, L))]
    Q = rng.integers(0, 256, (n, L), dtype=np.uint8)
    lens = np.full(n, L, np.int32) if full else rng.integers(1, L + 1, n).astype(np.int32)
    return np.ascontiguousarray(B), Q, lens


def text(i, k):
    """k name bytes without a space or a tab"""
    return bytes(33 + (i * 31 + j * 7) % 94 for j in range(k)).replace(b" ", b"x")


# ---------------------------------------------------------------- test 1: the place
PLACE_LENS = (15, 16, 17, 255, 256, 257, 700)


def place_names():
    names = [b" x", b"ab cd", b"abc ", b"a b c", b"abcd", b"", b"ab\tcd", b" ", b"\t", b"a"]
    for k in PLACE_LENS:
        t = text(k, k)
        names += [t, b" " + t[1:], t[:-1] + b" ", t[:k // 2] + b" " + t[k // 2 + 1:], t[:3] + b" " + t[4:k - 2] + b" " + t[k - 1:], t[:k // 2] + b"\t" + t[k // 2 + 1:]]
    return names


def check_place(codec, at):
    names = place_names()
    assert {len(x) for x in names} >= set(PLACE_LENS) | {0}
    n = len(names)
    B, Q, lens = rows(n, 40, seed=1)
    tag = Tag(np.zeros(n), np.full(n, 8), at=at)
    want = tagged_names(B, names, tag)
    if at == AT_SPACE:
        assert want[0] == b":" + bytes(B[0, :8]) + b" x" and want[3].startswith(b"a:") and want[3].endswith(b" b c") and want[5] == b":" + bytes(B[5, :8])
        assert want[6] == b"ab\tcd:" + bytes(B[6, :8]) and want[2].endswith(b" ") and want[2].startswith(b"abc:")
    else:
        assert all(w == x + b":" + bytes(B[i, :8]) for i, (w, x) in enumerate(zip(want, names)))
    for in_shift, out_shift in ((0, 0), (3, 9), (15, 1)):
        check(codec, B, Q, lens, names, tag, in_shift=in_shift, out_shift=out_shift, what="place at %d shifts %d %d" % (at, in_shift, out_shift))
    check(codec, B, Q, lens, names, Tag(np.zeros(n), np.full(n, 8), at=at, prefix=b"UMI", sep=b"#"), keep=(np.arange(n) % 3 != 1).astype(np.uint8), what="place at %d prefix" % at)


# ---------------------------------------------------------------- test 2: the seams of the blob
TILE = 4096


def seam_rows(out_shift=0):
    """names at the end of which (no space: X goes to the end) X straddles a tile boundary, then a head that ends exactly on one; short names behind them, some with
    spaces, so that X straddles 16-byte boundaries at every residue; the blob spans more than three tiles.  Tiles count from the 16-byte boundary at or below the
    blob, so the first name is out_shift bytes shorter for a blob that starts out_shift bytes behind one: both seams lie on tile edges at every alignment"""
    names = [text(0, 4090 - out_shift), text(1, TILE * 2 - 4099) + b" rest of the name"]
    names += [text(i, 5 + i % 29) + (b" 1:N:0" if i % 3 else b"") for i in range(2, 260)]
    n = len(names)
    B, Q, lens = rows(n, 24, seed=2)
    tag = Tag(np.arange(n) % 5, np.full(n, 8))
    return B, Q, lens, names, tag


def check_blob_seams(codec, out_shift):
    B, Q, lens, names, tag = seam_rows(out_shift)
    want = tagged_names(B, names, tag)
    off = np.concatenate([[0], np.cumsum([len(x) for x in want])]) + out_shift      # (positions from the 16-byte boundary at or below the blob: the tiles' own)
    assert off[-1] - out_shift > 3 * TILE
    # by construction, at every out_shift: X of name 0 is positions [4090, 4099) - across the tile boundary; the head of name 1 is positions [4099, 8192) - it ends on one
    assert off[0] + len(names[0]) == 4090 and off[1] == 4099 and off[1] + names[1].index(b" ") == 2 * TILE
    xs = [(int(off[i]) + (names[i].index(b" ") if b" " in names[i] else len(names[i])), 9) for i in range(len(names))]
    assert {(a % 16) for a, k in xs if a // 16 != (a + k - 1) // 16} >= set(range(8, 16)), "an X across a 16-byte boundary at every residue that crosses"
    check(codec, B, Q, lens, names, tag, out_shift=out_shift, in_shift=(out_shift * 7) % 16, what="blob seams shift %d" % out_shift)


def check_many_names_in_a_tile(codec):
    """more than 256 names start in one tile: names of 0 .. 3 bytes, a third of them untagged, some empty AND untagged"""
    n = 700
    names = [text(i, i % 4) for i in range(n)]
    B, Q, lens = rows(n, 8, seed=3)
    tlen = np.where(np.arange(n) % 3 == 0, 0, 1 + np.arange(n) % 2)
    tag = Tag(np.arange(n) % 4, tlen)
    want = tagged_names(B, names, tag)
    off = np.concatenate([[0], np.cumsum([len(x) for x in want])])
    assert int((off[:-1] < TILE).sum()) > 256 and sum(1 for x in want if not x) > 10
    for out_shift in (0, 5):
        check(codec, B, Q, lens, names, tag, out_shift=out_shift, what="many names in a tile")
    check(codec, B, Q, lens, names, Tag(tag.start, tag.length, at=AT_END), keep=(np.arange(n) % 7 != 2).astype(np.uint8), what="many names, some dropped, at end")


# ---------------------------------------------------------------- test 3: the parts
PART_LENS = (0, 1, 15, 16, 17, 32)


def check_parts(codec, codes):
    """every part length at the starts 0, 15, 16, 17 and lens - tag_len; a stride that is no multiple of 16, an unaligned buffer, and the last row's part is the last
    bytes of the allocation"""
    L = 50
    cases = [(ts, tl) for tl in PART_LENS for ts in (0, 15, 16, 17)] + [(None, tl) for tl in PART_LENS]
    cases = cases + cases[::-1][:5] + [(None, 32)]
    n = len(cases)
    B, Q, lens = rows(n, L, seed=4 + codes, codes=codes, full=False)
    lens = np.maximum(lens, 49).astype(np.int32); lens[-1] = L
    ts = np.array([int(lens[i]) - tl if s is None else s for i, (s, tl) in enumerate(cases)], np.int32); tl = np.array([c[1] for c in cases], np.int32)
    assert ts[-1] + tl[-1] == L and (ts + tl <= lens).all()
    names = [text(i, 9 + i % 11) + b" 2:N:0" for i in range(n)]
    tag = Tag(ts, tl)
    if not codes:
        P = b"".join(part(B, i, int(ts[i]), int(tl[i]), False) for i in range(n))
        assert any(c in P for c in b"acgt") and b"N" in P
    else:
        assert b"N" in b"".join(part(B, i, int(ts[i]), int(tl[i]), True) for i in range(n))
    start = np.minimum(lens, ts + tl).astype(np.int32)                        # (the window is independent of the part: behind it here, the whole read below)
    for in_shift in (0, 3):
        check(codec, B, Q, lens, names, tag, codes=codes, start=start, min_len=0, in_shift=in_shift, what="parts codes %d shift %d" % (codes, in_shift))
    check(codec, B, Q, lens, names, tag, codes=codes, in_shift=5, outputs="no", what="parts, names alone")


# ---------------------------------------------------------------- test 4: pairs
def check_pairs(codec):
    n = 40; L = 36
    B, Q, lens = rows(n, L, seed=6)
    names = [(text(i // 2, 12) + b" %d:N:0:ACGT" % (1 + i % 2)) for i in range(n)]
    tl = np.zeros(n, np.int32); ts = np.full(n, 2, np.int32)
    for u in range(n // 2):
        tl[2 * u], tl[2 * u + 1] = ((8, 6), (8, 0), (0, 6), (0, 0))[u % 4]
    keep = np.ones(n, np.uint8); length = np.full(n, 20, np.int32); start = np.full(n, 10, np.int32)
    length[9] = 3                                                            # R2 of pair 4 (both parts) is short: the pair gives no name
    keep[16] = 0                                                             # R1 of pair 8 (both parts) is masked
    for prefix, join in ((b"", b"_"), (b"UMI", b"_"), (b"RX", b"+")):
        tag = Tag(ts, tl, prefix=prefix, join=join)
        want = tagged_names(B, names, tag, pairs=True)
        x0 = b":" + (prefix + join if prefix else b"") + bytes(B[0, 2:10]) + join + bytes(B[1, 2:8])
        assert want[0] == names[0][:12] + x0 + names[0][12:] and want[1] == names[1][:12] + x0 + names[1][12:]
        assert want[2] == names[2][:12] + b":" + (prefix + join if prefix else b"") + bytes(B[2, 2:10]) + names[2][12:] and want[6] == names[6] and want[7] == names[7]
        assert want[5] == names[5][:12] + b":" + (prefix + join if prefix else b"") + bytes(B[5, 2:8]) + names[5][12:]
        r = check(codec, B, Q, lens, names, tag, keep=keep, start=start, length=length, pairs=True, min_len=10, what="pairs prefix %r join %r" % (prefix, join))
        assert r[0] == n - 4 and r[6:] == (1, 1, 2)
        check(codec, B, Q, lens, names, tag, pairs=False, what="the same arrays, rows alone")


# ---------------------------------------------------------------- test 5: identity
def check_identity(codec):
    """a tag whose parts are all empty gives byte for byte what no tag gives: rows, lens, names, offsets and result"""
    n = 300
    B, Q, lens = rows(n, 33, seed=7, full=False)
    names = [text(i, i % 41) + (b" x" if i % 2 else b"") for i in range(n)]
    keep = (np.arange(n) % 5 != 3).astype(np.uint8)
    for pairs in (False, True):
        plain = run(codec, B, Q, lens, names, None, keep=keep, pairs=pairs, out_shift=3)
        for path in PATHS:
            codec.set_option(OPTION, path)
            try:
                got = run(codec, B, Q, lens, names, Tag(np.zeros(n), np.zeros(n), prefix=b"UMI"), keep=keep, pairs=pairs, out_shift=3)
            finally:
                codec.set_option(OPTION, None)
            assert got == plain, "a tag of empty parts changed the call (option %s)" % path


# ---------------------------------------------------------------- test 6: sizes
def check_sizes(codec):
    from repaq_amd import RfqError
    n = 120
    B, Q, lens = rows(n, 20, seed=8)
    names = [text(i, 3 + i % 26) + b" r" for i in range(n)]
    tag = Tag(np.full(n, 1), 4 + np.arange(n) % 9, prefix=b"U")
    keep = (np.arange(n) % 7 != 3).astype(np.uint8)
    e = S.expected(B, Q, lens, tagged_names(B, names, tag), keep)
    m, nl = len(e["idx"]), e["names_len"]
    assert e["max_name"] == max(len(x) for x in e["names"]) > max(len(x) for x in names)
    dev = dev_tag(codec, B, Q, lens, names, tag, keep)
    g = dict(n=W.Guarded(codec, nl), o=W.Guarded(codec, 8 * (m + 1)))
    try:
        for path in PATHS:
            codec.set_option(OPTION, path)
            kw = dict(tag=tag_of(dev, tag), **S.sel_of(dev))
            before = {k: v.body() for k, v in g.items()}
            with R.pytest_raises(RfqError) as ei:
                codec.select_rows(*dev.args(), row_len=20, out_names=g["n"].ptr, names_cap=nl - 1, out_name_off=g["o"].ptr, off_cap=m + 1, **kw)
            assert ei.value.code == E_NOSPACE and "need" in ei.value.message and "%d name bytes" % nl in ei.value.message, ei.value
            assert all(v.body() == before[k] and v.guards_intact() for k, v in g.items())
            r = codec.select_rows(*dev.args(), row_len=20, out_names=g["n"].ptr, names_cap=nl, out_name_off=g["o"].ptr, off_cap=m + 1, **kw)
            assert (r.n_rows, r.names_len, r.max_name) == (m, nl, e["max_name"]) and g["n"].body() == b"".join(e["names"]) and all(v.guards_intact() for v in g.values())
            # no row is kept: nothing but the one offset
            none = dev_tag(codec, B, Q, lens, names, tag, np.zeros(n, np.uint8))
            try:
                r = codec.select_rows(*none.args(), row_len=20, out_names=g["n"].ptr, names_cap=nl, out_name_off=g["o"].ptr, off_cap=m + 1, tag=tag_of(none, tag), **S.sel_of(none))
                assert (r.n_rows, r.names_len, r.max_name, r.dropped_mask) == (0, 0, 0, n) and g["o"].body()[:8] == b"\0" * 8 and all(v.guards_intact() for v in g.values())
            finally:
                none.free()
    finally:
        codec.set_option(OPTION, None)
        dev.free()
        for v in g.values():
            v.free()
    check(codec, B[:0], Q[:0], lens[:0], [], Tag([], []), what="no rows at all")
    # no rows and NULL arrays (what an empty tensor hands over): the call of no rows, as the plain one
    zero = codec.dev_put(b"\0" * 8)
    try:
        for path in PATHS:
            codec.set_option(OPTION, path)
            r = codec.select_rows(0, 20, None, None, None, None, 0, zero, tag=dict(d_tag_start=None, d_tag_len=None, prefix=b"UMI"))
            assert result_of(r) == (0,) * 9
    finally:
        codec.set_option(OPTION, None)
        codec.dev_free(zero)


# ---------------------------------------------------------------- test 7: refusals
def _good(codec):
    """what every refusal is followed by, on the same context: a PLAIN select that matches the model"""
    S._good(codec)


def check_host_refusals(codec):
    from repaq_amd import RfqError
    n, L = 12, 24
    B, Q, lens = rows(n, L, seed=9)
    names = [text(i, 7) for i in range(n)]
    tag = Tag(np.zeros(n), np.full(n, 4))
    dev = dev_tag(codec, B, Q, lens, names, tag)
    buf = codec.dev_put(b"\0" * 4096); b = buf.value
    try:
        rows_named = dev.args(); rows_bare = (n, L, dev.bases, dev.quals, dev.lens)

        def at(p, k):
            return C.c_void_p(p.value + k)

        def T(raw=None, **kw):
            d = tag_of(dev, tag, raw); d.update(kw); return d
        sel = codec.select_rows
        out_names = dict(row_len=L, out_names=C.c_void_p(b), names_cap=4096)
        calls = (("take no tag", lambda: sel(*rows_bare, tag=T())),
                 ("null d_tag_start / d_tag_len", lambda: sel(*rows_named, tag=T(d_tag_start=None))),
                 ("null d_tag_start / d_tag_len", lambda: sel(*rows_named, tag=T(d_tag_len=None))),
                 ("4-byte aligned", lambda: sel(*rows_named, tag=T(d_tag_start=at(dev.tstart, 2)))),
                 ("4-byte aligned", lambda: sel(*rows_named, tag=T(d_tag_len=at(dev.tlen, 1)))),
                 ("prefix_len is at most 14", lambda: sel(*rows_named, tag=T(prefix=b"A" * 15))),
                 ("null h_prefix", lambda: sel(*rows_named, tag=T(raw=dict(prefix_len=3)))),
                 ("sep and join", lambda: sel(*rows_named, tag=T(sep=b" "))),
                 ("sep and join", lambda: sel(*rows_named, tag=T(sep=b"\x7f"))),
                 ("sep and join", lambda: sel(*rows_named, tag=T(join=b"\n"))),
                 ("sep and join", lambda: sel(*rows_named, tag=T(join=b"\x80"))),
                 ("the prefix holds a byte outside 0x21..0x7E (0x20 at 2)", lambda: sel(*rows_named, tag=T(prefix=b"UM I"))),
                 ("the prefix holds a byte outside", lambda: sel(*rows_named, tag=T(prefix=b"\tU"))),
                 ("at must be", lambda: sel(*rows_named, tag=T(at=2))),
                 ("bad base_mode", lambda: sel(*rows_named, tag=T(), base_mode=7)),
                 ("null rows->d_bases", lambda: sel(n, L, None, dev.quals, dev.lens, dev.names, dev.names_len, dev.name_off, tag=T())),
                 ("d_names overlaps the input tag->d_tag_start", lambda: sel(*rows_named, tag=T(), row_len=L, out_names=at(dev.tstart, 4), names_cap=16)),
                 ("d_lens overlaps the input tag->d_tag_len", lambda: sel(*rows_named, tag=T(), row_len=L, out_lens=dev.tlen, lens_cap=n)),
                 ("d_name_off overlaps the input tag->d_tag_len", lambda: sel(*rows_named, tag=T(), row_len=L, out_name_off=at(dev.tlen, 8 - dev.tlen.value % 8), off_cap=2)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == E_ARG and what in ei.value.message, (what, ei.value)
            _good(codec)
        # (without the tag the same rows pass - a bad base_mode is not looked at, the base rows are not needed -, and so does a tag into a buffer of the caller's own)
        assert sel(*rows_named, base_mode=7).n_rows == n and sel(n, L, None, dev.quals, dev.lens, dev.names, dev.names_len, dev.name_off).n_rows == n
        assert sel(*rows_named, tag=T(prefix=b"A" * 14), **out_names).names_len == n * (7 + 1 + 15 + 4)
    finally:
        dev.free(); codec.dev_free(buf)


def _device_refusals():
    """(label, error code, mutation(ts, tl, lens, B, row))"""
    I32 = 0x7FFFFFFF

    def st(v):
        return lambda ts, tl, lens, B, r: ts.__setitem__(r, v)

    def ln(v):
        return lambda ts, tl, lens, B, r: tl.__setitem__(r, v)

    def both(a, b):
        return lambda ts, tl, lens, B, r: (ts.__setitem__(r, a(lens[r]) if callable(a) else a), tl.__setitem__(r, b))
    return [("start_minus_1", E_ARG, st(-1)), ("len_minus_1", E_ARG, ln(-1)), ("len_33", E_ARG, ln(33)), ("ends_one_behind_the_read", E_ARG, both(lambda l: int(l) - 3, 4)),
            ("start_and_len_int_max", E_ARG, both(I32, I32)), ("start_int_max_len_0", E_ARG, both(I32, 0)),
            ("bad_part_byte", E_DATA, lambda ts, tl, lens, B, r: B.__setitem__((r, int(ts[r]) + int(tl[r]) - 1), 0xFF)),
            # (0x20: below 0x21 as a letter - what a pad or a space would be - and above 4 as a code; the part's FIRST byte, so the last stays good)
            ("space_as_part_byte", E_DATA, lambda ts, tl, lens, B, r: B.__setitem__((r, int(ts[r])), 0x20))]


DEVICE_REFUSALS = _device_refusals()
DEVICE_REFUSAL_IDS = [r[0] for r in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    """the offence in the LAST row, in a DROPPED row, and in two rows (the first is named) - rows alone and pairs, letters and codes; nothing is written; a plain
    select follows"""
    from repaq_amd import RfqError
    _, code, mutate = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    n, L = 300, 21
    names = [text(i, 4 + i % 9) for i in range(n)]
    for codes, pairs, where in ((False, False, "last"), (True, True, "last"), (False, True, "dropped"), (True, False, "two")):
        B, Q, lens = rows(n, L, seed=10, codes=codes, full=False)
        B = B.copy(); lens = np.maximum(lens, 8).astype(np.int32)
        ts = np.ones(n, np.int32); tl = np.full(n, 5, np.int32); keep = np.ones(n, np.uint8)
        bad = dict(last=[n - 1], dropped=[77], two=[123, 40])[where]
        for r in bad:
            mutate(ts, tl, lens, B, r)
        if where == "dropped":
            keep[77] = 0
        tag = Tag(ts, tl)
        dev = dev_tag(codec, B, Q, lens, names, tag, keep, shift=1)
        g = [W.Guarded(codec, n * L), W.Guarded(codec, 4 * n), W.Guarded(codec, dev.names_len + 12 * n), W.Guarded(codec, 8 * (n + 1))]
        try:
            before = [x.body() for x in g]
            for path in PATHS:
                codec.set_option(OPTION, path)
                for query in (True, False):
                    out = {} if query else dict(row_len=L, out_bases=g[0].ptr, bases_cap=n * L, out_lens=g[1].ptr, lens_cap=n, out_names=g[2].ptr, names_cap=g[2].n,
                                                out_name_off=g[3].ptr, off_cap=n + 1)
                    with R.pytest_raises(RfqError) as ei:
                        codec.select_rows(*dev.args(), pairs=pairs, codes=codes, tag=tag_of(dev, tag), **S.sel_of(dev), **out)
                    assert ei.value.code == code and "first such row: %d)" % min(bad) in ei.value.message and "tag part" in ei.value.message, (label, where, ei.value)
                    assert [x.body() for x in g] == before and all(x.guards_intact() for x in g)
            codec.set_option(OPTION, None)
            _good(codec)
        finally:
            codec.set_option(OPTION, None)
            dev.free()
            for x in g:
                x.free()


# ---------------------------------------------------------------- test 8: state
def check_state(codec):
    """tagged, plain, tagged with a smaller batch, on one context: the scratch is reused and nothing of the earlier call is seen"""
    big = rows(900, 30, seed=11); small = rows(37, 30, seed=12)
    nb = [text(i, 20 + i % 50) + b" 1:N" for i in range(900)]; ns = [text(i, 3 + i % 5) for i in range(37)]
    for path in PATHS:
        codec.set_option(OPTION, path)
        try:
            run(codec, *big, nb, Tag(np.arange(900) % 7, np.full(900, 12), prefix=b"UMI"), pairs=True, what="state: the large tagged call")
            run(codec, *big, nb, None, what="state: the plain call")
            run(codec, *small, ns, Tag(np.zeros(37), 1 + np.arange(37) % 3), what="state: the small tagged call")
            run(codec, *big, nb, Tag(np.arange(900) % 7, np.full(900, 12), prefix=b"UMI"), pairs=True, what="state: the large tagged call again")
        finally:
            codec.set_option(OPTION, None)


def check_stage_names(codec):
    """select:tagplan and select:names come back through the timings of a tagged call, the plan only on the default formulation; a plain call has no plan"""
    B, Q, lens = rows(50, 20, seed=13)
    names = [text(i, 9) for i in range(50)]
    tag = Tag(np.zeros(50), np.full(50, 6))
    run(codec, B, Q, lens, names, tag)
    t = [k for k, _ in codec.timings()]
    assert t == ["select:judge", "select:tables", "select:rows", "select:tagplan", "select:names"], t
    codec.set_option(OPTION, "general")
    try:
        run(codec, B, Q, lens, names, tag)
        assert [k for k, _ in codec.timings()] == ["select:judge", "select:tables", "select:rows", "select:names"]
    finally:
        codec.set_option(OPTION, None)
    run(codec, B, Q, lens, names, None)
    assert [k for k, _ in codec.timings()] == ["select:judge", "select:tables", "select:rows", "select:names"]


# ---------------------------------------------------------------- test 9: the switch
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


# ---------------------------------------------------------------- test 10: composition with tensors (the GPU twin)
def compose_text(pairs=70, seed=21):
    """two paired FASTQ texts with inline UMIs (8 bases and 2 linker bases in front of both mates), Illumina-style names; a few reads shorter than the UMI, a few
    with a lower-case base or an N inside it"""
    rng = np.random.default_rng(seed)
    t1, t2 = [], []
    for p in range(pairs):
        recs = []
        for m in (1, 2):
            k = int(rng.integers(12, 60))
            if p % 17 == 3 and m == 1:
                k = 5                                                         # shorter than the UMI: the tag is the 5 bases, nothing is left of the read
            if p % 19 == 4 and m == 2:
                k = 9                                                         # the UMI and one linker base
            s = bytearray(b"ACGT"[int(x)] for x in rng.integers(0, 4, k))
            if p % 7 == 2:
                s[3] = ord("N")
            if p % 11 == 5 and m == 2:
                s[1] = ord("a")
            q = bytes(b"F:,#5"[int(x)] for x in rng.integers(0, 5, k))
            recs.append((b"@M01:23:FC:1:%d:%d:%d %d:N:0:ACGT" % (1101 + p // 9, 1000 + 7 * p, 2000 + 3 * p, m), bytes(s), q))
        t1.append(recs[0]); t2.append(recs[1])
    return t1, t2


def fastq(recs):
    return b"".join(b"%s\n%s\n+\n%s\n" % r for r in recs)


def compose_expected(t1, t2, umi_len=8, umi_skip=2, prefix=b"UMI", starts=None, min_len=1):
    """the two texts extract_umi(loc="per_read", pairs=True) and rows_to_fastq leave, by the rules: both names take sep, prefix, "_", R1's UMI, "_" if both have one,
    R2's UMI in front of their first space; the UMI and umi_skip bases leave each read; a pair one of whose reads has fewer than min_len bases left is dropped.
    starts: where each read's UMI begins (None: 0), reads in row order.  Returns (text 1, text 2, pairs dropped, the tagged names of the kept rows)"""
    o1, o2, dropped, kept = [], [], 0, []
    for p, (a, b) in enumerate(zip(t1, t2)):
        umis, cuts = [], []
        for m, (name, s, q) in enumerate((a, b)):
            ts = 0 if starts is None else int(starts[2 * p + m])
            u = s[ts:ts + umi_len]
            umis.append(u); cuts.append(min(len(s), ts + len(u) + umi_skip))
        T = (b"_" if all(umis) else b"").join(umis)
        X = b":" + (prefix + b"_" if prefix else b"") + T if T else b""
        if any(len(r[1]) - c < min_len for r, c in zip((a, b), cuts)):
            dropped += 1
            continue
        for (name, s, q), c, o in zip((a, b), cuts, (o1, o2)):
            at = name.index(b" ")
            tagged = name[:at] + X + name[at:]
            kept.append(tagged)
            o.append((tagged, s[c:], q[c:]))
    return fastq(o1), fastq(o2), dropped, kept
