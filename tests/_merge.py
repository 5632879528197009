"""Shared helpers of the rfq_merge_rows tests (tests/test_emu_merge.py on the SIMT interpreter, tests/test_gpu_merge.py on the MI355X).

Nothing expected comes from the code under test: merge_pair() restates the rules of include/rfq_hip.h as a plain loop over the fragment's positions p, expected()
calls it per merged pair and adds up the counts.  Every output goes into a _rows.Guarded buffer of exactly the reported size, and the guards are checked after each
call.  Every check runs under RFQ_MERGE default and general and compares bases, quals, lens, names, offsets and the result struct byte for byte."""
import ctypes as C

import numpy as np

import _adapter as A
import _rows as W
import _rows_enc as R

PAD_B, PAD_Q = 0xA7, 0x51
PATHS = (None, "general")
FIELDS = ("n_rows", "n_bases", "names_len", "max_len", "max_name", "n_pairs", "overlap_bases")
COMP_ASCII = {65: 84, 84: 65, 67: 71, 71: 67, 97: 116, 116: 97, 99: 103, 103: 99}


# ---------------------------------------------------------------- the rules, as loops
def comp(c, codes):
    """rfq_adapter_rows' complement as a byte map"""
    if codes:
        return 3 - c if c < 4 else c
    return COMP_ASCII.get(c, c)


def cls(c, codes):
    """0 .. 3 = A C G T, 4 = other"""
    return (c if c < 4 else 4) if codes else int(A.ASCII_CLASS[c])


def merge_pair(r1, q1, r2, q2, ins, codes):
    """(bases, quals, positions both mates cover, those of them that do not agree) of one pair; r1 / q1 / r2 / q2: the reads' own bytes, their lengths l1 / l2"""
    l1, l2 = len(r1), len(r2)
    assert l1 >= 1 and l2 >= 1 and 1 <= ins <= l1 + l2 - 1, (l1, l2, ins)
    ob, oq, both, differ = bytearray(), bytearray(), 0, 0
    for p in range(ins):
        c1 = p < min(l1, ins); c2 = p >= ins - l2
        assert c1 or c2
        if c2:
            i = ins - 1 - p
            b2, s2 = comp(int(r2[i]), codes), int(q2[i])
        if c1:
            b1, s1 = int(r1[p]), int(q1[p])
        if c1 and c2:
            both += 1
            k1, k2 = cls(b1, codes), cls(b2, codes)
            if k1 < 4 and k1 == k2:                                          # 1. they agree
                b, s = b1, max(s1, s2)
            else:
                differ += 1
                if (k1 < 4) != (k2 < 4):                                     # 2. exactly one of them is in A C G T
                    b, s = (b1, s1) if k1 < 4 else (b2, s2)
                elif s1 >= s2:                                               # 3. otherwise
                    b, s = b1, s1 - s2
                else:
                    b, s = b2, s2 - s1
        elif c1:
            b, s = b1, s1
        else:
            b, s = b2, s2
        ob.append(b); oq.append(s)
    return bytes(ob), bytes(oq), both, differ


def expected(B, Q, lens, names, insert, codes):
    """dict of what rfq_merge_rows must report and write (rows as lists of byte strings: the stride is the caller's)"""
    n = len(lens); insert = np.asarray(insert, np.int64)
    assert n % 2 == 0 and len(insert) == n // 2
    idx = np.nonzero(insert >= 0)[0]
    e = dict(idx=idx, bases=[], quals=[], differ=[], overlap=0, n_pairs=n // 2, lens=insert[idx].astype(np.int32),
             names=None if names is None else [names[2 * k] for k in idx])
    for k in idx:
        l1, l2 = int(lens[2 * k]), int(lens[2 * k + 1])
        b, q, both, differ = merge_pair(B[2 * k, :l1], Q[2 * k, :l1], B[2 * k + 1, :l2], Q[2 * k + 1, :l2], int(insert[k]), codes)
        e["bases"].append(b); e["quals"].append(q); e["differ"].append(differ); e["overlap"] += both
    e["max_len"] = int(e["lens"].max()) if len(idx) else 0
    e["n_bases"] = int(e["lens"].sum())
    e["names_len"] = sum(map(len, e["names"])) if names is not None else 0
    e["max_name"] = max(map(len, e["names"])) if names is not None and len(idx) else 0
    e["result"] = (len(idx), e["n_bases"], e["names_len"], e["max_len"], e["max_name"], n // 2, e["overlap"])
    return e


# ---------------------------------------------------------------- calling
def dev_merge(codec, B, Q, lens, names, insert, shift=0, name_off=None):
    """_rows.DevRows with the pairs' insert sizes as its extra input: dev.insert"""
    return W.DevRows(codec, B, Q, lens, names, shift=shift, name_off=name_off, insert=(insert, np.int32))


def out_len(ml, rule):
    """the output stride: None exactly max_len, "x16" the next multiple of 16 + 16, an int as given"""
    if rule is None:
        return max(ml, 1)
    return (ml + 15) // 16 * 16 + 16 if rule == "x16" else int(rule)


def result_of(r):
    return tuple(int(getattr(r, f)) for f in FIELDS)


def call(codec, B, Q, lens, names, insert, codes, row_len=None, in_shift=0, out_shift=0, outputs="bqlno", paths=PATHS, e=None):
    """Per path one size query and one rfq_merge_rows into Guarded buffers of exactly the reported sizes (_rows.compact_into_guarded), compared with expected();
    both paths must write the same bytes.  Returns (expected dict, bases, quals, raw bytes of every output body) of the last path."""
    e = e or expected(B, Q, lens, names, insert, codes)
    dev = dev_merge(codec, B, Q, lens, names, insert, shift=in_shift)
    if names is None:
        outputs = outputs.replace("n", "").replace("o", "")
    kw = dict(d_insert=dev.insert, codes=codes)
    n = len(e["idx"])

    def rows_differ(kind, g, wantr, bad):
        j = int(bad[0]); k = int(e["idx"][j]); at = int(np.nonzero(g[j] != wantr[j])[0][0])
        return "%s rows differ: %d of %d, first %d (pair %d: l1 %d, l2 %d, insert %d) at position %d: got %r, want %r" % (
            kind, len(bad), n, j, k, lens[2 * k], lens[2 * k + 1], insert[k], at, bytes(g[j][at:at + 8]), bytes(wantr[j][at:at + 8]))
    raws = []
    try:
        for path in paths:
            codec.set_option("RFQ_MERGE", path)
            what = "path %s: " % (path or "default")
            q = codec.merge_rows(*dev.args(), **kw)
            assert result_of(q) == e["result"], (what, result_of(q), e["result"])
            r, gB, gQ, _, raw = W.compact_into_guarded(codec, lambda **out: codec.merge_rows(*dev.args(), **out, **kw), e, out_len(e["max_len"], row_len),
                                                       PAD_B, PAD_Q, outputs, out_shift, what, rows_differ)
            assert result_of(r) == e["result"], (what, result_of(r), e["result"])
            raws.append(raw)
        assert all(x == raws[0] for x in raws), "the two formulations wrote different bytes"
        return e, gB, gQ, raws[-1]
    finally:
        codec.set_option("RFQ_MERGE", None)
        dev.free()


# ---------------------------------------------------------------- making pairs
CODE_ALPHABET = np.array([0, 1, 2, 3, 0, 1, 2, 3, 4, 7, 255], np.uint8)
ASCII_ALPHABET = np.frombuffer(b"ACGTACGTacgtNnRY.", np.uint8)


def random_pairs(npairs, L, seed, codes, full=False):
    """npairs pairs of stride L: lengths 1 .. L (full: all L), bases of every class, scores of every value with many ties, noise behind the reads; every third
    pair has insert -1, the others a random valid one"""
    rng = np.random.default_rng(seed)
    n = 2 * npairs
    lens = np.full(n, L, np.int32) if full else rng.integers(1, L + 1, n).astype(np.int32)
    alpha = CODE_ALPHABET if codes else ASCII_ALPHABET
    B = alpha[rng.integers(0, len(alpha), (n, L))]
    Q = np.where(rng.random((n, L)) < 0.3, 30, rng.integers(0, 256, (n, L))).astype(np.uint8)
    for k in range(npairs):                                                  # (make most overlaps agree mostly: R2 = the reverse complement of R1's bytes at a shift)
        if k % 2 == 0:
            l1, l2 = int(lens[2 * k]), int(lens[2 * k + 1]); m = min(l1, l2)
            B[2 * k + 1, :m] = [comp(int(c), codes) for c in B[2 * k, :m][::-1]]
    inside = np.arange(L)[None, :] < lens[:, None]
    B = np.where(inside, B, rng.integers(0, 256, (n, L))).astype(np.uint8); Q = np.where(inside, Q, rng.integers(0, 256, (n, L))).astype(np.uint8)
    insert = np.array([-1 if k % 3 == 2 else int(rng.integers(1, int(lens[2 * k]) + int(lens[2 * k + 1]))) for k in range(npairs)], np.int32)
    for k in range(0, npairs, 2):
        if insert[k] >= 0 and k % 4 == 0:
            insert[k] = min(int(lens[2 * k]), int(lens[2 * k + 1]))         # (the shift at which the planted agreement lies, for equal lengths)
    names = [b"@p%d/%d" % (i // 2, i % 2 + 1) + b"x" * (i % 7) for i in range(n)]
    return B, Q, lens, names, insert


# ---------------------------------------------------------------- test 1: shapes
ROW_LENS = (1, 15, 16, 17, 33, 64, 152, 260)


def check_shapes(codec, L):
    for codes in (True, False):
        B, Q, lens, names, insert = random_pairs(36, L, 100 + L, codes)
        e = expected(B, Q, lens, names, insert, codes)
        assert 0 < len(e["idx"]) < 36
        for shift in (0, 1):
            for rule in (None, "x16"):
                call(codec, B, Q, lens, names, insert, codes, row_len=rule, in_shift=shift, out_shift=shift, e=e)


# ---------------------------------------------------------------- test 2: every insert
EVERY_INSERT = ((1, 1), (16, 16), (20, 20), (17, 33), (33, 17), (40, 5), (5, 40))
EVERY_INSERT_IDS = ["%d_%d" % x for x in EVERY_INSERT]


def r2_load_edges(L, npairs, lens, insert):
    """(the reversed 16-byte load of pair 0 starts in front of the buffer, that of the last pair ends behind it) for some group that holds bytes of R2"""
    front = back = False
    for k in (0, npairs - 1):
        l1, l2, ins = int(lens[2 * k]), int(lens[2 * k + 1]), int(insert[k])
        for k0 in range(0, ins, 16):
            if max(k0, ins - l2) < min(k0 + 16, ins):                        # (R2 covers a position of the group)
                start = (2 * k + 1) * L + ins - 16 - k0
                front |= k == 0 and start < 0
                back |= k == npairs - 1 and start + 16 > 2 * npairs * L
    return front, back


def check_every_insert(codec, label):
    l1, l2 = EVERY_INSERT[EVERY_INSERT_IDS.index(label)]
    L = max(l1, l2); npairs = l1 + l2 - 1
    edges = []
    for codes, shift in ((True, 0), (True, 1), (False, 1)):
        B, Q, lens, names, _ = random_pairs(npairs, L, 200 + 41 * l1 + l2, codes, full=True)
        lens[0::2] = l1; lens[1::2] = l2
        insert = np.arange(1, npairs + 1, dtype=np.int32)
        assert int(insert[0]) - l2 <= 0 <= int(insert[-1]) - l2 and int(insert[-1]) == l1 + l2 - 1 and (l1 == 1 or int(insert[0]) < l1)      # both signs of d; R1's tail left out
        edges.append(r2_load_edges(L, npairs, lens, insert))
        for rule in (None, "x16"):
            call(codec, B, Q, lens, names, insert, codes, row_len=rule, in_shift=shift, out_shift=shift)
    return edges[0]


def check_load_edges_are_reached():
    """among test 2's cases: one whose pair 0 has its reversed load start in front of the buffer, one whose last pair has it end behind the buffer"""
    got = []
    for l1, l2 in EVERY_INSERT:
        n = l1 + l2 - 1
        lens = np.empty(2 * n, np.int32); lens[0::2] = l1; lens[1::2] = l2
        got.append(r2_load_edges(max(l1, l2), n, lens, np.arange(1, n + 1)))
    assert any(f for f, _ in got) and any(b for _, b in got), got


# ---------------------------------------------------------------- test 3: the consensus table
A_, C_, G_, T_, N_ = 0, 1, 2, 3, 4
# (R1's class, the class of comp(R2's base)) at q1 = 30, q2 = 12 -> (the base's source, the score), written out by hand from the three rules
HAND = {(A_, A_): (1, 30), (C_, C_): (1, 30), (G_, G_): (1, 30), (T_, T_): (1, 30),           # 1. agree: r1, max
        (A_, C_): (1, 18), (A_, G_): (1, 18), (A_, T_): (1, 18), (C_, G_): (1, 18), (C_, T_): (1, 18), (G_, T_): (1, 18),      # 3. two different bases, q1 >= q2: r1, q1 - q2
        (N_, N_): (1, 18),                                                                   # 3. two others
        (A_, N_): (1, 30), (C_, N_): (1, 30), (G_, N_): (1, 30), (T_, N_): (1, 30),           # 2. only R1's is a base: r1, q1
        (N_, A_): (2, 12), (N_, C_): (2, 12), (N_, G_): (2, 12), (N_, T_): (2, 12)}           # 2. only R2's is a base: b2, q2
SCORES = ((30, 12), (12, 30), (30, 30), (0, 0), (0, 255), (255, 0), (255, 255), (0, 1), (255, 254))
TABLE_INS = 40
TABLE_POS = (0, 15, 16, TABLE_INS - 1)


def check_consensus_table(codec, codes):
    syms = [0, 1, 2, 3, 4] if codes else list(b"ACGTNacgtR")
    cases = [(x, y, s, p) for x in syms for y in syms for s in SCORES for p in TABLE_POS]
    npairs = len(cases); L = TABLE_INS
    bg = 0 if codes else ord("A")
    B = np.full((2 * npairs, L), bg, np.uint8); Q = np.full((2 * npairs, L), 20, np.uint8)
    B[1::2] = comp(bg, codes)
    for k, (x, y, (s1, s2), p) in enumerate(cases):
        i = TABLE_INS - 1 - p
        B[2 * k, p] = x; Q[2 * k, p] = s1
        B[2 * k + 1, i] = comp(y, codes); Q[2 * k + 1, i] = s2                # (so that comp(r2[i]) == y)
    lens = np.full(2 * npairs, L, np.int32); insert = np.full(npairs, TABLE_INS, np.int32)
    e, gB, gQ, _ = call(codec, B, Q, lens, None, insert, codes, row_len="x16")
    assert e["overlap"] == npairs * TABLE_INS
    seen = set()
    for k, (x, y, s, p) in enumerate(cases):
        if s != (30, 12):
            continue
        key = (cls(x, codes), cls(y, codes))
        src, score = HAND[key] if key in HAND else HAND[key[::-1]]           # (the other order of two different bases is the same case: r1 wins on its score)
        if key not in HAND:
            assert key[0] < 4 and key[1] < 4 and key[0] != key[1]
        want = (x if src == 1 else y, score)
        assert (int(gB[k, p]), int(gQ[k, p])) == want, (codes, x, y, p, (int(gB[k, p]), int(gQ[k, p])), want)
        seen.add(tuple(sorted(key)))
    assert len(seen) == 15                                                   # (the fifteen class pairs)
    return npairs


# ---------------------------------------------------------------- test 4: an oracle that does not share the rule's code
FRAG_L = 150
FRAG_CRIT = A.crit(pairs=True, min_overlap=20, max_diff=5, max_diff_pct=20)
FRAG_FOUND_UP_TO = 2 * FRAG_L - 30
FILLER = (np.array([0, 2, 0, 3, 1, 2, 2, 0, 0, 2, 0, 2, 1] * 12, np.uint8), np.array([1, 3, 2, 3, 1, 3, 1, 3, 3, 0, 3, 0, 1] * 12, np.uint8))


def fragments(npairs=120, seed=4):
    """pairs read from random fragments F of 20 .. 299 bases (codes): R1 = F[:150], R2 = revcomp(F)[:150], adapter filler behind a short fragment; score 40
    everywhere but at up to three errors planted in one mate, which have score 5.  Returns (B, Q, lens, names, list of F)."""
    rng = np.random.default_rng(seed); l = FRAG_L
    B = np.zeros((2 * npairs, l), np.uint8); Q = np.full((2 * npairs, l), 40, np.uint8); F = []
    for k in range(npairs):
        f = int(rng.integers(20, 300)) if k >= 6 else (20, 29, 150, 151, 270, 299)[k]
        fr = rng.integers(0, 4, f).astype(np.uint8); F.append(fr)
        for m, x in ((0, fr), (1, A.rc(fr))):
            B[2 * k + m] = np.concatenate([x, FILLER[m]])[:l]
        m = int(rng.integers(0, 2)); lo, hi = max(0, f - l), min(f, l)        # fragment positions [lo, hi) are read twice: an error there can be mended
        for p in rng.choice(np.arange(lo, hi), size=min(int(rng.integers(0, 4)), hi - lo), replace=False):
            at = int(p) if m == 0 else f - 1 - int(p)
            B[2 * k + m, at] = (int(B[2 * k + m, at]) + int(rng.integers(1, 4))) & 3; Q[2 * k + m, at] = 5
    names = [b"@frag.%d/%d" % (i // 2, i % 2 + 1) for i in range(2 * npairs)]
    return B, Q, np.full(2 * npairs, l, np.int32), names, F


def check_fragments_result(F, insert, diff, e, gB):
    """what test 4 asserts of the adapter call's insert / diff and the merged rows"""
    found = np.nonzero(np.asarray(insert) >= 0)[0]
    planted = [k for k, fr in enumerate(F) if len(fr) <= FRAG_FOUND_UP_TO]
    assert len(planted) > len(F) // 2 and set(planted) <= set(int(k) for k in found), "the adapter call missed a planted pair"
    assert any(len(F[k]) < FRAG_L for k in found) and any(len(F[k]) > FRAG_L for k in found)
    for j, k in enumerate(found):
        fr = F[int(k)]
        assert int(insert[k]) == len(fr), (k, int(insert[k]), len(fr))
        assert bytes(gB[j, :len(fr)]) == bytes(fr), "merged row %d (pair %d) is not its fragment" % (j, k)
        assert e["differ"][j] == int(diff[k]), (k, e["differ"][j], int(diff[k]))
    assert sum(e["differ"]) > 0


def check_fragments(codec):
    B, Q, lens, names, F = fragments()
    n = len(lens)
    dev = W.DevRows(codec, B, None, lens)
    gi, gd = W.Guarded(codec, 2 * n), W.Guarded(codec, 2 * n)
    try:
        codec.adapter_rows(*dev.adapter_args(), codes=True, d_insert=gi.ptr, d_diff=gd.ptr, **FRAG_CRIT)
        insert = np.frombuffer(gi.body(), np.int32).copy(); diff = np.frombuffer(gd.body(), np.int32).copy()
    finally:
        dev.free(); gi.free(); gd.free()
    e, gB, _, _ = call(codec, B, Q, lens, names, insert, True)
    check_fragments_result(F, insert, diff, e, gB)


# ---------------------------------------------------------------- test 5: nothing, everything, degenerate
def check_degenerate(codec):
    B, Q, lens, names, insert = random_pairs(10, 20, 5, True)
    e, _, _, raw = call(codec, B[:0], Q[:0], lens[:0], [], insert[:0], True)                    # no rows at all
    assert e["result"] == (0,) * 7 and raw[4] == bytes(8)
    e, _, _, raw = call(codec, B, Q, lens, names, np.full(10, -1, np.int32), True)              # no pair merged
    assert e["result"] == (0, 0, 0, 0, 0, 10, 0) and raw[4] == bytes(8) and raw[0] == b""
    call(codec, B, Q, lens, names, np.full(10, -7, np.int32), True, outputs="o")
    every = np.where(insert < 0, 1, insert).astype(np.int32)
    e = call(codec, B, Q, lens, names, every, True, row_len="x16")[0]                           # every pair merged
    assert e["result"][0] == 10
    for ins in (1, int(lens[0]) + int(lens[1]) - 1, -1):                                        # one pair alone
        call(codec, B[:2], Q[:2], lens[:2], names[:2], np.array([ins], np.int32), True)


# ---------------------------------------------------------------- test 6: names
NAME_LENS = (0, 1, 15, 16, 17, 300)


def check_names(codec):
    npairs = 4 * len(NAME_LENS)
    B, Q, lens, _, insert = random_pairs(npairs, 24, 6, False)
    names = []
    for k in range(npairs):
        nl = NAME_LENS[(k // 2) % len(NAME_LENS)]                         # (every third pair is not merged: the lengths go by in twos)
        names += [bytes(33 + (k * 31 + i) % 90 for i in range(nl)), b"@R2-of-%d-must-not-appear" % k]
    for in_shift, out_shift in ((0, 0), (1, 1), (7, 3)):
        e, _, _, raw = call(codec, B, Q, lens, names, insert, False, in_shift=in_shift, out_shift=out_shift)
        assert b"must-not-appear" not in raw[3] and {len(x) for x in e["names"]} == set(NAME_LENS)
    e = call(codec, B, Q, lens, None, insert, False)[0]                                         # rows without names
    assert e["result"][2] == e["result"][4] == 0
    from repaq_amd import RfqError
    dev = dev_merge(codec, B, Q, lens, None, insert)
    g = W.Guarded(codec, 4096)
    try:
        for kw in (dict(out_names=g.ptr, names_cap=4096), dict(out_name_off=g.ptr, off_cap=512)):
            with R.pytest_raises(RfqError) as ei:
                codec.merge_rows(*dev.args(), d_insert=dev.insert, row_len=64, **kw)
            assert ei.value.code == -3, ei.value
    finally:
        dev.free(); g.free()


# ---------------------------------------------------------------- test 7: outputs
def _good(codec):
    """what every refusal is followed by, on the same context"""
    B, Q, lens, names, insert = random_pairs(12, 20, 9, True)
    call(codec, B, Q, lens, names, insert, True, paths=(None,))


def check_outputs(codec):
    from repaq_amd import RfqError
    B, Q, lens, names, insert = random_pairs(60, 37, 7, False)
    e, _, _, raw = call(codec, B, Q, lens, names, insert, False)
    assert call(codec, B, Q, lens, names, insert, False, e=e)[3] == raw, "the same call on the same context wrote other bytes"
    for k, o in enumerate("bqlno"):                                          # each output alone
        got = call(codec, B, Q, lens, names, insert, False, outputs=o, row_len="x16" if o in "bq" else None, e=e)[3]
        assert o in "bq" or got == [raw[k]], o                               # (the rows at another stride: compared inside call())
    n, nl, L = len(e["idx"]), e["names_len"], e["max_len"]
    dev = dev_merge(codec, B, Q, lens, names, insert)
    g = dict(b=W.Guarded(codec, n * L), q=W.Guarded(codec, n * L), l=W.Guarded(codec, 4 * n), n=W.Guarded(codec, nl), o=W.Guarded(codec, 8 * (n + 1)))
    try:
        caps = dict(bases_cap=n * L, quals_cap=n * L, lens_cap=n, names_cap=nl, off_cap=n + 1)
        ptrs = dict(out_bases=g["b"].ptr, out_quals=g["q"].ptr, out_lens=g["l"].ptr, out_names=g["n"].ptr, out_name_off=g["o"].ptr, d_insert=dev.insert)
        before = {k: v.body() for k, v in g.items()}
        for path in PATHS:
            codec.set_option("RFQ_MERGE", path)
            for short in list(caps) + ["row_len"]:                           # (row_len = max_len - 1 is refused too)
                kw = dict(caps, row_len=L); kw[short] -= 1
                with R.pytest_raises(RfqError) as ei:
                    codec.merge_rows(*dev.args(), **ptrs, **kw)
                assert ei.value.code == -8 and "need" in ei.value.message, (short, ei.value)
                assert all(v.body() == before[k] and v.guards_intact() for k, v in g.items()), short
            codec.set_option("RFQ_MERGE", None)
            _good(codec)
        r = codec.merge_rows(*dev.args(), **ptrs, row_len=L, pad_base=PAD_B, pad_qual=PAD_Q, **caps)
        assert result_of(r) == e["result"] and [g[k].body() for k in "bqlno"] == raw and all(v.guards_intact() for v in g.values())
    finally:
        codec.set_option("RFQ_MERGE", None)
        dev.free()
        for v in g.values():
            v.free()


# ---------------------------------------------------------------- test 8: refusals
def check_host_refusals(codec):
    from repaq_amd import RfqError
    npairs, L = 20, 16; n = 2 * npairs
    B, Q, lens, names, insert = random_pairs(npairs, L, 12, True)
    dev = dev_merge(codec, B, Q, lens, names, insert)
    buf = codec.dev_put(b"\0" * (1 << 16)); b = buf.value
    try:
        M = codec.merge_rows; rows = dev.args(); ins = dict(d_insert=dev.insert)
        out = dict(row_len=2 * L, out_bases=C.c_void_p(b), bases_cap=npairs * 2 * L)

        def at(p, k):
            return C.c_void_p(p.value + k)
        calls = (("odd n_rows", lambda: M(n - 1, L, dev.bases, dev.quals, dev.lens, **ins)),
                 ("no d_insert", lambda: M(*rows)),
                 ("misaligned d_insert", lambda: M(*rows, d_insert=at(dev.insert, 2))),
                 ("misaligned out d_lens", lambda: M(*rows, **ins, row_len=2 * L, out_lens=C.c_void_p(b + 2), lens_cap=1000)),
                 ("misaligned in d_lens", lambda: M(n, L, dev.bases, dev.quals, at(dev.lens, 2), dev.names, dev.names_len, dev.name_off, **ins)),
                 ("misaligned out d_name_off", lambda: M(*rows, **ins, row_len=2 * L, out_name_off=C.c_void_p(b + 4), off_cap=1000)),
                 ("misaligned in d_name_off", lambda: M(n, L, dev.bases, dev.quals, dev.lens, dev.names, dev.names_len, at(dev.name_off, 4), **ins)),
                 ("row_len 0", lambda: M(*rows, **ins, row_len=0, out_bases=C.c_void_p(b), bases_cap=1 << 16)),
                 ("bad base_mode", lambda: M(*rows, **ins, base_mode=2)),
                 ("no bases with bases wanted", lambda: M(n, L, None, dev.quals, dev.lens, dev.names, dev.names_len, dev.name_off, **ins, **out)),
                 ("no quals with quals wanted", lambda: M(n, L, dev.bases, None, dev.lens, dev.names, dev.names_len, dev.name_off, **ins, row_len=2 * L,
                                                          out_quals=C.c_void_p(b), quals_cap=npairs * 2 * L)),
                 ("bases out on bases in", lambda: M(*rows, **ins, row_len=L, out_bases=dev.bases, bases_cap=npairs * L)),
                 ("quals out ends in quals in", lambda: M(*rows, **ins, row_len=L, out_quals=C.c_void_p(dev.quals.value - npairs * L + 1), quals_cap=npairs * L)),
                 ("lens out on lens in", lambda: M(*rows, **ins, row_len=L, out_lens=dev.lens, lens_cap=npairs)),
                 ("lens out on d_insert", lambda: M(*rows, **ins, row_len=L, out_lens=dev.insert, lens_cap=npairs)),
                 ("names out inside names in", lambda: M(*rows, **ins, row_len=L, out_names=at(dev.names, 5), names_cap=dev.names_len)),
                 ("bases out on the last offset in", lambda: M(*rows, **ins, row_len=L, out_bases=at(dev.name_off, 8 * n + 7), bases_cap=npairs * L)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == -3, (what, ei.value)
            _good(codec)
        r = M(*rows, **ins, **out)                                           # (a buffer of the caller's own that lies on nothing is taken)
        assert r.n_pairs == npairs and r.n_rows == int((insert >= 0).sum())
    finally:
        dev.free(); codec.dev_free(buf)


DEVICE_REFUSALS = ("negative_length", "length_above_row_len", "insert_0", "insert_l1_plus_l2", "l1_0_with_an_insert", "name_offsets_decrease",
                   "last_offset_past_names_len", "bad_length_in_a_pair_that_is_not_merged")


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    npairs, L = 30, 24; n = 2 * npairs
    B, Q, lens, names, insert = random_pairs(npairs, L, 13, True)
    lens = np.maximum(lens, 3).astype(np.int32)
    insert = np.where(insert >= 0, 2, -1).astype(np.int32)                   # (valid for every pair)
    name_off = None; nl_delta = 0
    if label == "negative_length":
        lens[17] = -1; needle = "first such row: 17)"
    elif label == "length_above_row_len":
        lens[44] = L + 1; needle = "first such row: 44)"
    elif label == "insert_0":
        insert[4] = 0; needle = "first such pair: 4)"
    elif label == "insert_l1_plus_l2":
        insert[9] = int(lens[18]) + int(lens[19]); needle = "first such pair: 9)"
    elif label == "l1_0_with_an_insert":
        lens[12] = 0; insert[6] = 1; needle = "first such pair: 6)"
    elif label == "name_offsets_decrease":
        name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint64); name_off[[12, 13]] = name_off[[13, 12]]
        needle = "first such row: 12)"
    elif label == "last_offset_past_names_len":
        nl_delta = -1; needle = "first such row: %d)" % (n - 1)
    else:
        assert insert[5] == -1
        lens[11] = L + 7; needle = "first such row: 11)"
    dev = dev_merge(codec, B, Q, lens, names, insert, name_off=name_off)
    g = [W.Guarded(codec, npairs * 2 * L), W.Guarded(codec, npairs * 2 * L), W.Guarded(codec, 4 * npairs), W.Guarded(codec, dev.names_len), W.Guarded(codec, 8 * (npairs + 1))]
    try:
        args = list(dev.args()); args[6] += nl_delta
        before = [x.body() for x in g]
        for path in PATHS:
            codec.set_option("RFQ_MERGE", path)
            for query in (True, False):
                out = {} if query else dict(row_len=2 * L, out_bases=g[0].ptr, bases_cap=npairs * 2 * L, out_quals=g[1].ptr, quals_cap=npairs * 2 * L, out_lens=g[2].ptr,
                                            lens_cap=npairs, out_names=g[3].ptr, names_cap=dev.names_len, out_name_off=g[4].ptr, off_cap=npairs + 1)
                with R.pytest_raises(RfqError) as ei:
                    codec.merge_rows(*args, d_insert=dev.insert, codes=True, **out)
                assert ei.value.code == -3 and needle in ei.value.message, (label, ei.value)
                assert [x.body() for x in g] == before and all(x.guards_intact() for x in g)
            codec.set_option("RFQ_MERGE", None)
            _good(codec)
    finally:
        codec.set_option("RFQ_MERGE", None)
        dev.free()
        for x in g:
            x.free()


# ---------------------------------------------------------------- test 9: the switch and the timings
def check_switch_and_timings(codec):
    import _engine as E
    from repaq_amd import RfqError
    assert "RFQ_MERGE" in codec.option_names()
    codec.set_option("RFQ_MERGE", "general")
    assert codec.get_option("RFQ_MERGE") == "general"
    E.reset_options(codec)
    assert codec.get_option("RFQ_MERGE") == ""
    codec.set_option("RFQ_MERGE", "staged")
    with R.pytest_raises(RfqError):
        codec.set_option("RFQ_MERGE", "fast")
    B, Q, lens, names, insert = random_pairs(8, 40, 1, True)
    call(codec, B, Q, lens, names, insert, True, paths=(None,))
    t = codec.timings()
    assert [x for x, _ in t] == ["merge:judge", "merge:tables", "merge:rows", "merge:names"] and all(np.isfinite(ms) for _, ms in t), t


# ---------------------------------------------------------------- test 10: text -> adapter -> merge -> text
COMPOSE_A = A.crit(pairs=True, min_overlap=20, max_diff=3, max_diff_pct=10)


def compose_expected(t1, t2):
    """(the merged text, the two texts of the pairs that are not merged, merged pairs, the adapter step's reference) of _adapter.compose_text()'s records"""
    recs = [x for pair in zip(t1, t2) for x in pair]
    rows = [rec.split(b"\n")[:4] for rec in recs]
    L = max(len(r[1]) for r in rows); n = len(rows)
    B = np.zeros((n, L), np.uint8); Q = np.zeros((n, L), np.uint8); lens = np.array([len(r[1]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        B[i, :lens[i]] = np.frombuffer(r[1], np.uint8); Q[i, :lens[i]] = np.frombuffer(r[3], np.uint8) - 33
    ea = A.expected(B, lens, COMPOSE_A, False)
    e = expected(B, Q, lens, [r[0] for r in rows], ea["insert"], False)
    merged = b"".join(nm + b"\n" + b + b"\n+\n" + bytes(x + 33 for x in q) + b"\n" for nm, b, q in zip(e["names"], e["bases"], e["quals"]))
    rest = [b"".join(recs[2 * k + m] for k in range(n // 2) if ea["insert"][k] < 0) for m in (0, 1)]
    assert 50 < len(e["idx"]) < n // 2 - 20, len(e["idx"])
    return merged, rest[0], rest[1], len(e["idx"]), ea


def check_composition(codec):
    from repaq_amd import PE_TWO_FILES, SE
    t1, t2 = A.compose_text()
    merged, w1, w2, m, ea = compose_expected(t1, t2)
    _, B, Q, lens, names = codec.text_rows_bytes(b"".join(t1), b"".join(t2), paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    dev = W.DevRows(codec, B, Q, lens, names)
    gi = W.Guarded(codec, 2 * n)
    bufs = []
    try:
        a = codec.adapter_rows(n, 160, dev.bases, dev.lens, d_insert=gi.ptr, **COMPOSE_A)
        assert A.summary_of(a) == ea["summary"] and gi.guards_intact()
        rows = dev.args(); kw = dict(d_insert=gi.ptr, codes=False)
        q = codec.merge_rows(*rows, **kw)
        assert int(q.n_rows) == m
        L, nl = max(int(q.max_len), 1), int(q.names_len)
        ob, oq, ol, on, oo = (codec.dev_put(b"\0" * max(k, 1)) for k in (m * L, m * L, 4 * m, nl, 8 * (m + 1)))
        bufs += [ob, oq, ol, on, oo]
        codec.merge_rows(*rows, row_len=L, out_bases=ob, bases_cap=m * L, out_quals=oq, quals_cap=m * L, out_lens=ol, lens_cap=m, out_names=on, names_cap=nl,
                         out_name_off=oo, off_cap=m + 1, **kw)
        r = codec.rows_to_text(m, L, ob, oq, ol, on, nl, oo, paired=SE, qual_offset=33)
        assert codec.dev_get(r.d_fq1, r.n1) == merged, "the merged text differs from the host's"
    finally:
        dev.free(); gi.free()
        for p in bufs:
            codec.dev_free(p)
