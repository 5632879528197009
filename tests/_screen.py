"""Shared helpers of the rfq_screen_build / rfq_screen_rows tests (tests/test_emu_screen.py on the SIMT interpreter, tests/test_gpu_screen.py on the MI355X).

Nothing expected comes from the code under test: the set is a Python `set` of canonical ints built straight from the rules of include/rfq_hip.h - a k-mer is a
string of base-4 digits, its value int(s, 4), its reverse complement the reversed string with the digits complemented -, a row's k-mers and hits a plain loop over
its positions, the verdict the two integer comparisons.  Every comparison is exact integer equality.  Every output goes into a _rows.Guarded buffer of exactly as
many entries as the call may write, and the guards are checked after each call."""
import ctypes as C

import numpy as np

import _rows as W
import _rows_enc as R

BUILD_FIELDS = ("n_refs", "ref_bases", "n_positions", "n_kmers", "slots", "index_bytes")
FIELDS = ("n_units", "n_candidates", "n_matched", "n_kept", "kmers", "hits", "bases_in", "bases_kept")
OPTION = "RFQ_SCREEN"
PATHS = (None, "general")
BUILDS = (None, "general", "collide")
E_ARG, E_DATA, E_NOSPACE = -3, -5, -8

# ---------------------------------------------------------------- the reference
ASCII_DIGIT = bytearray(b"x" * 256)
CODE_DIGIT = bytearray(b"x" * 256)
for _i, _b in enumerate(b"ACGT"):
    ASCII_DIGIT[_b] = ASCII_DIGIT[_b | 0x20] = CODE_DIGIT[_i] = ord("0") + _i
ASCII_DIGIT, CODE_DIGIT = bytes(ASCII_DIGIT), bytes(CODE_DIGIT)
COMP = bytes.maketrans(b"0123", b"3210")


def digits(b, codes):
    """the classes of a sequence as a string of the digits 0 .. 3, x for "other\""""
    return bytes(b).translate(CODE_DIGIT if codes else ASCII_DIGIT)


def canon(s):
    """the canonical value of the k-mer whose classes are the digit string s, None when it is not valid"""
    if b"x" in s:
        return None
    return min(int(s, 4), int(s[::-1].translate(COMP), 4))


def kmers_of(d, k):
    """the canonical values of the valid k-mers of the digit string d, position by position"""
    for p in range(len(d) - k + 1):
        v = canon(d[p:p + k])
        if v is not None:
            yield v


def ref_set(refs, k):
    """(the set, the number of valid k-mers) of a list of reference sequences: no k-mer spans two of them"""
    s, n = set(), 0
    for r in refs:
        for v in kmers_of(digits(r, False), k):
            s.add(v); n += 1
    return s, n


def slots_of(refs_len):
    s = 1024
    while s < 2 * refs_len:
        s *= 2
    return s


def expected(B, lens, S, k, codes, pairs=False, cand=None, min_hits=1, min_pct=0, keep_matched=False):
    """what rfq_screen_rows must write and report: kmers [n], hits [n], keep [n] as numpy arrays and the summary as a dict"""
    n = len(lens); nr = 2 if pairs else 1; U = n // nr
    kmers = np.zeros(n, np.uint32); hits = np.zeros(n, np.uint32); keep = np.zeros(n, np.uint8)
    s = dict.fromkeys(FIELDS, 0); s["n_units"] = U
    Bb = [bytes(r) for r in np.ascontiguousarray(B)]
    for u in range(U):
        rows = range(nr * u, nr * u + nr)
        if cand is not None and not all(int(cand[g]) for g in rows):
            continue
        for g in rows:
            vs = list(kmers_of(digits(Bb[g][:int(lens[g])], codes), k))
            kmers[g] = len(vs); hits[g] = sum(v in S for v in vs)
        K = sum(int(kmers[g]) for g in rows); H = sum(int(hits[g]) for g in rows); bases = sum(int(lens[g]) for g in rows)
        matched = H >= max(min_hits, 1) and 100 * H >= min_pct * K
        kept = matched if keep_matched else not matched
        keep[nr * u:nr * u + nr] = kept
        s["n_candidates"] += 1; s["n_matched"] += matched; s["n_kept"] += kept; s["kmers"] += K; s["hits"] += H; s["bases_in"] += bases; s["bases_kept"] += bases if kept else 0
    return dict(kmers=kmers, hits=hits, keep=keep, summary=s)


# ---------------------------------------------------------------- sequences
LETTERS = np.frombuffer(b"ACGT", np.uint8)
RC_ASCII = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rand_seq(rng, n):
    return bytes(LETTERS[rng.integers(0, 4, n)])


def revcomp(s):
    return bytes(s)[::-1].translate(RC_ASCII)


def as_mode(s, mode):
    """an upper-case ASCII sequence in the row's form: "ascii", "lower" or "code" (every letter that is not one of ACGT becomes code 4)"""
    if mode == "ascii":
        return bytes(s)
    if mode == "lower":
        return bytes(s).lower()
    return bytes(W.CODE[np.frombuffer(bytes(s), np.uint8)].clip(0, 4))


def rows_of(seqs, L=None, mode="ascii", pad=None, seed=1):
    """(B [n, L] uint8, lens) of a list of upper-case ASCII sequences in `mode`; behind a read lies `pad` (None: noise)"""
    n = len(seqs); L = L or max([len(s) for s in seqs] + [1])
    B = np.random.default_rng(seed).integers(0, 256, (n, L), dtype=np.uint8) if pad is None else np.full((n, L), pad, np.uint8)
    for i, s in enumerate(seqs):
        B[i, :len(s)] = np.frombuffer(as_mode(s, mode), np.uint8)
    return B, np.array([len(s) for s in seqs], np.int32)


# ---------------------------------------------------------------- the calls
def summary_of(r, fields=FIELDS):
    return {f: int(getattr(r, f)) for f in fields}


class Index:
    """an index built by rfq_screen_build from a list of reference sequences (bytes), in a Guarded buffer of exactly index_bytes, beside the model's set; the
    build's result is compared with the model's counts.  option: the value of RFQ_SCREEN the build runs under."""
    def __init__(self, codec, refs, k, option=None):
        refs = [bytes(r) for r in refs]
        self.codec, self.k, self.refs = codec, k, refs
        self.set, self.n_positions = ref_set(refs, k)
        blob = b"".join(refs); off = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.uint64)
        self.refs_len, self.n_refs = len(blob), len(refs)
        self.d_blob = codec.dev_put(blob); self.d_off = codec.dev_put(off.tobytes())
        self.g = None
        codec.set_option(OPTION, option)
        try:
            q = codec.screen_build(*self.src(), k=k, size_only=True)
            want = slots_of(len(blob))
            assert (int(q.slots), int(q.index_bytes)) == (want, 64 + 8 * want), (summary_of(q, BUILD_FIELDS), want)
            self.bytes = int(q.index_bytes)
            self.g = W.Guarded(codec, self.bytes)
            self.result = self.build()
        except Exception:
            self.free()
            raise
        finally:
            codec.set_option(OPTION, None)

    def src(self):
        return (self.d_blob, self.refs_len, self.d_off, self.n_refs)

    def build(self):
        """the build into this index's buffer (again): the counts are the model's every time"""
        r = self.codec.screen_build(*self.src(), k=self.k, d_index=self.g.ptr, index_cap=self.bytes)
        assert self.g.guards_intact(), "a guard around the index was written"
        got = summary_of(r, BUILD_FIELDS)
        want = dict(n_refs=self.n_refs, ref_bases=self.refs_len, n_positions=self.n_positions, n_kmers=len(self.set), slots=(self.bytes - 64) // 8, index_bytes=self.bytes)
        assert got == want, {f: (got[f], want[f]) for f in BUILD_FIELDS if got[f] != want[f]}
        return got

    @property
    def ptr(self):
        return self.g.ptr

    def free(self):
        if self.g is not None:
            self.g.free()
        self.codec.dev_free(self.d_blob); self.codec.dev_free(self.d_off)


def dev_rows(codec, B, lens, cand=None, shift=0):
    return W.DevRows(codec, B, None, lens, shift=shift, cand=(cand, np.uint8))


NAMES = dict(n="kmers", h="hits", k="keep")
DTYPES = dict(n=np.uint32, h=np.uint32, k=np.uint8)
OUT_ARGS = dict(n="d_kmers", h="d_hits", k="d_keep")


def run(codec, dev, idx, codes=False, pairs=False, min_hits=1, min_pct=0, keep_matched=False, outputs="nhk", index=None):
    """one rfq_screen_rows into Guarded buffers of exactly the entries the call may write; returns (dict of numpy outputs, summary dict, raw bytes of the outputs).
    index: (pointer, bytes) of another index than idx's own"""
    n = dev.n
    sizes = dict(n=4 * n, h=4 * n, k=n)
    g = {o: W.Guarded(codec, sizes[o]) for o in outputs}
    ptr, nbytes = index if index is not None else (idx.ptr, idx.bytes)
    try:
        r = codec.screen_rows(*dev.adapter_args(), ptr, nbytes, codes=codes, pairs=pairs, min_hits=min_hits, min_pct=min_pct, keep_matched=keep_matched, d_in=dev.cand,
                              **{OUT_ARGS[o]: g[o].ptr for o in outputs})
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


def check(codec, B, lens, idx, codes=False, pairs=False, cand=None, min_hits=1, min_pct=0, keep_matched=False, shifts=(0,), paths=PATHS, outputs="nhk", what=""):
    """the call equals the reference, at every shift and on every path; returns the reference"""
    e = expected(B, lens, idx.set, idx.k, codes, pairs, cand, min_hits, min_pct, keep_matched)
    for shift in shifts:
        dev = dev_rows(codec, B, lens, cand, shift)
        try:
            for path in paths:
                codec.set_option(OPTION, path)
                out, summ, _ = run(codec, dev, idx, codes, pairs, min_hits, min_pct, keep_matched, outputs)
                compare(out, summ, e, "%s shift %d option %s:" % (what, shift, path or "default"))
        finally:
            codec.set_option(OPTION, None)
            dev.free()
    return e


# ---------------------------------------------------------------- test 1: every position, every k
KS = (4, 15, 16, 17, 31)
MODES = ("ascii", "lower", "code")
BACKGROUND = b"AC" * 24                                                       # 48 bases with two k-mers, ACAC.. and CACA..


def apart_reference(k, seed):
    """a reference of k + 40 random bases that shares no k-mer with BACKGROUND (asserted: the test does not rest on luck)"""
    bg = set(kmers_of(digits(BACKGROUND, False), k))
    for t in range(1000):
        ref = rand_seq(np.random.default_rng(1000 * seed + t), k + 40)
        if not (ref_set([ref], k)[0] & bg):
            return ref
    raise AssertionError("no reference apart from the background")


def check_every_position(codec, k):
    """ONE reference k-mer at every start 0 .. 48 - k of a 48-base row: hits as the model says - at least the planted one -, kmers = l - k + 1; the background
    alone has none; the same rows reverse-complemented hit as often"""
    ref = apart_reference(k, k)
    idx = Index(codec, [ref], k)
    try:
        seqs = [BACKGROUND]
        for s in range(48 - k + 1):
            j = s % 41
            seqs.append(BACKGROUND[:s] + ref[j:j + k] + BACKGROUND[s + k:])
        assert all(len(x) == 48 for x in seqs)
        for mode in MODES:
            codes = mode == "code"
            for rows in (seqs, [revcomp(x) for x in seqs]):
                B, lens = rows_of(rows, 48, mode)
                e = check(codec, B, lens, idx, codes=codes, shifts=(0, 5), what="k %d %s" % (k, mode))
                assert e["hits"][0] == 0 and (e["hits"][1:] >= 1).all() and (e["kmers"] == 48 - k + 1).all(), (k, mode, list(e["hits"]))
    finally:
        idx.free()


# ---------------------------------------------------------------- test 2: validity
def check_validity(codec):
    rng = np.random.default_rng(52)
    for k, mode in ((4, "ascii"), (16, "code"), (17, "lower"), (31, "ascii")):
        codes = mode == "code"
        ref = rand_seq(rng, 48)
        idx = Index(codec, [ref], k)
        try:
            # an "other" byte at every position removes exactly the k-mers that cover it
            seqs = [ref] + [ref[:p] + b"N" + ref[p + 1:] for p in range(48)]
            B, lens = rows_of(seqs, 48, mode)
            if codes:
                for p in range(0, 48, 3):
                    B[1 + p, p] = (4, 5, 255)[p % 3]                         # (any code above 3)
            e = check(codec, B, lens, idx, codes=codes, what="an other byte, k %d" % k)
            full = 48 - k + 1
            for p in range(48):
                covered = min(p, full - 1) - max(p - k + 1, 0) + 1
                assert e["kmers"][1 + p] == full - covered and e["hits"][1 + p] == full - covered, (k, p, e["kmers"][1 + p], e["hits"][1 + p])
            assert e["kmers"][0] == full and e["hits"][0] == full
            # l < k, l == k, l == 0 - and the reference's own bytes behind the read are padding: never counted
            B = np.tile(np.frombuffer(as_mode(ref, mode), np.uint8), (6, 1)); lens = np.array([0, 1, k - 1, k, k + 1, 48], np.int32)
            e = check(codec, B, lens, idx, codes=codes, shifts=(0, 1), what="short rows, k %d" % k)
            assert list(e["kmers"]) == [0, 0, 0, 1, 2, full] and list(e["hits"]) == [0, 0, 0, 1, 2, full]
        finally:
            idx.free()
    # a k-mer that is its own reverse complement
    own = b"ACGT" * 4
    assert revcomp(own) == own
    idx = Index(codec, [own], 16)
    try:
        assert len(idx.set) == 1
        B, lens = rows_of([b"TTTTT" + own + b"GGGGGGG", own, b"T" + own[:-1] + b"C"], 32, "ascii")
        e = check(codec, B, lens, idx, what="self-complementary")
        assert list(e["hits"]) == [1, 1, 0] and list(e["kmers"]) == [13, 1, 2]
    finally:
        idx.free()


# ---------------------------------------------------------------- test 3: seams
SEAM_LENS = (15, 16, 17, 255, 256, 257, 1023, 1024, 1025, "2049+k")
SEAM_IDS = [str(x) for x in SEAM_LENS]


def check_seams(codec, label):
    """reference k-mers across every 16-byte lane boundary (and with it the 256 and 1024 kernel limits and the long kernel's tile seam at 1024: the starts
    1024 - k .. 1024): row (phase, r) carries one at b - r, r = 0 .. k, for every multiple b of 16 with b / 16 % 3 == phase (48 bases apart: no plant lies on
    another), in a random background; rows at their own alignment"""
    k = 31 if label in ("1024", "2049+k") else (4 if label in ("15", "16", "17") else 17)
    L = 2049 + k if label == "2049+k" else int(label)
    rng = np.random.default_rng(53 + L)
    ref = rand_seq(rng, k + 40)
    idx = Index(codec, [ref], k)
    try:
        seqs = []
        for phase in (1, 0, 2):                                              # (1024 / 16 % 3 == 1: rows 0 .. k carry the tile seam's)
            for r in range(k + 1):
                s = bytearray(rand_seq(rng, L))
                for b in range(16, L + 16, 16):
                    at = b - r
                    if 0 <= at and at + k <= L and (b // 16) % 3 == phase:
                        j = (b // 16 + r) % 41
                        s[at:at + k] = ref[j:j + k]
                seqs.append(bytes(s))
        for mode, shifts in (("ascii", (0, 3)), ("code", (9,))):
            B, lens = rows_of(seqs, L, mode)
            lens[1::5] = rng.integers(0, L + 1, len(lens[1::5]))             # (a few shorter reads: the seam behind the read's end)
            e = check(codec, B, lens, idx, codes=mode == "code", shifts=shifts, what="seams L %d %s" % (L, mode))
            assert e["summary"]["hits"] > 0 and e["summary"]["hits"] < e["summary"]["kmers"]
            if L >= 1024 + k:
                assert all(e["hits"][r] >= 64 // 3 for r in range(k + 1) if lens[r] == L)
    finally:
        idx.free()


SC_ITER = 4                                                                    # (enc/rows_screen.h)


def check_walk(codec, label):
    """unit counts around a wave, a step and a workgroup (the walk of the device-memory placement: 256 threads, SC_ITER steps) and around the LDS placement's step
    of 1024 threads, rows and pairs, against a small index (LDS) and a large one (device memory)"""
    L, path, counts = W.walk_case(label, SC_ITER)
    lpr = 16 if L <= 256 else 64
    counts = sorted(set(counts) | ({1024 // lpr - 1, 1024 // lpr, 1024 // lpr + 1, 4 * 1024 // lpr + 1} if L <= 1024 and path is None else set()))
    rng = np.random.default_rng(54 + L)
    k = 15
    ref = rand_seq(rng, 600)
    small, large = Index(codec, [ref], k), Index(codec, [ref, rand_seq(rng, 8200)], k)
    try:
        assert small.bytes == 64 + 8 * 2048 and large.bytes == 64 + 8 * 32768
        for U in counts:
            for pairs in (False, True):
                n = (2 if pairs else 1) * U
                seqs = []
                for i in range(n):
                    l = int(rng.integers(0, 41)) if i % 4 else 40
                    s = bytearray(rand_seq(rng, l))
                    if i % 3 == 0 and l >= 20:
                        j = int(rng.integers(0, 580)); s[3:3 + 17] = ref[j:j + 17]
                    seqs.append(bytes(s))
                B, lens = rows_of(seqs, L, "ascii", pad=ord("A"))
                B[:, L - 16:] = np.frombuffer(ref[:16], np.uint8)             # (the row's last lane holds bytes, none of them inside a read)
                for idx in (small, large):
                    e = check(codec, B, lens, idx, pairs=pairs, shifts=(n % 16,), paths=(path,), what="walk L %d units %d pairs %d" % (L, U, pairs))
                    assert U < 3 or e["summary"]["n_matched"] >= 1
    finally:
        small.free(); large.free()


def check_walk_bad_length(codec):
    """a bad length in the last row, a workgroup's first unit behind its last step: the refusal names it"""
    from repaq_amd import RfqError
    rng = np.random.default_rng(55)
    small, large = Index(codec, [rand_seq(rng, 100)], 15), Index(codec, [rand_seq(rng, 8200)], 15)
    try:
        for idx, threads in ((small, 1024), (large, 256)):
            for L in (256, 272):
                n = threads // (16 if L <= 256 else 64) * SC_ITER + 1
                B, lens = rows_of([rand_seq(rng, 30)] * n, L)
                lens[n - 1] = L + 1
                dev = dev_rows(codec, B, lens)
                try:
                    with R.pytest_raises(RfqError) as ei:
                        run(codec, dev, idx)
                    assert ei.value.code == E_ARG and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
                finally:
                    dev.free()
    finally:
        small.free(); large.free()


# ---------------------------------------------------------------- test 4: the verdict
def check_verdict(codec):
    k = 16
    ref = apart_reference(k, 56)
    idx = Index(codec, [ref], k)
    try:
        def row(h):
            """35 bases, K = 20: h >= 1 reference k-mers in front (h + k - 1 reference bases), background behind"""
            o = 1 if h and ref[h + k - 1] == BACKGROUND[0] else 0             # (the background does not go on as the reference does)
            s = ref[:h + k - 1] + BACKGROUND[o:o + 35 - (h + k - 1)] if h else BACKGROUND[:35]
            assert len(s) == 35
            return s
        seqs = [row(5), row(4), row(0), row(1), row(20)]
        B, lens = rows_of(seqs, 40, "ascii")
        e0 = expected(B, lens, idx.set, k, False)
        assert list(e0["kmers"]) == [20] * 5 and list(e0["hits"]) == [5, 4, 0, 1, 20], (list(e0["kmers"]), list(e0["hits"]))
        for keep_matched in (False, True):
            for min_hits, min_pct, matched in ((0, 0, [1, 1, 0, 1, 1]), (1, 0, [1, 1, 0, 1, 1]), (5, 0, [1, 0, 0, 0, 1]), (6, 0, [0, 0, 0, 0, 1]),
                                               (1, 25, [1, 0, 0, 0, 1]),       # 100 * 5 == 25 * 20; one hit fewer: 400 < 500
                                               (1, 26, [0, 0, 0, 0, 1]), (1, 20, [1, 1, 0, 0, 1]), (1, 100, [0, 0, 0, 0, 1]), (21, 100, [0, 0, 0, 0, 0])):
                e = check(codec, B, lens, idx, min_hits=min_hits, min_pct=min_pct, keep_matched=keep_matched, shifts=(0, 2), what="verdict %d %d" % (min_hits, min_pct))
                assert list(e["keep"]) == [m if keep_matched else 1 - m for m in matched], (min_hits, min_pct, keep_matched, list(e["keep"]))
                assert e["summary"]["n_matched"] == sum(matched) and e["summary"]["bases_kept"] == 35 * int(e["keep"].sum())
        # pairs: the sums are taken over both mates - a hit only in R2 drops R1 too; 100 * 5 >= 12 * 40 but < 13 * 40
        P = [row(0), row(5), row(5), row(0), row(0), row(0), row(1), row(4)]
        B, lens = rows_of(P, 40, "ascii")
        for min_hits, min_pct, matched in ((1, 0, [1, 1, 0, 1]), (1, 12, [1, 1, 0, 1]), (1, 13, [0, 0, 0, 0]), (5, 0, [1, 1, 0, 1]), (6, 0, [0, 0, 0, 0])):
            for keep_matched in (False, True):
                e = check(codec, B, lens, idx, pairs=True, min_hits=min_hits, min_pct=min_pct, keep_matched=keep_matched, what="pairs %d %d" % (min_hits, min_pct))
                assert list(e["keep"][0::2]) == list(e["keep"][1::2]) == [m if keep_matched else 1 - m for m in matched], (min_hits, min_pct, list(e["keep"]))
        # candidates: a row that is none gets 0 / 0 / 0 in either mode, a failing mate fails the pair; any non-zero byte counts
        cand = np.array([1, 1, 0, 7, 255, 1, 1, 0], np.uint8)
        for pairs in (False, True):
            for keep_matched in (False, True):
                e = check(codec, B, lens, idx, pairs=pairs, cand=cand, keep_matched=keep_matched, shifts=(0, 1), what="candidates pairs %d" % pairs)
                out = np.array([0, 0, 1, 1, 0, 0, 1, 1], bool) if pairs else cand == 0
                assert not e["keep"][out].any() and not e["kmers"][out].any() and not e["hits"][out].any()
                assert e["summary"]["n_candidates"] == (2 if pairs else 6) and (e["kmers"][~out] == 20).all()
        e = check(codec, B, lens, idx, pairs=True, cand=np.zeros(8, np.uint8), what="no candidates")
        assert e["summary"] == dict(dict.fromkeys(FIELDS, 0), n_units=4)
        # each output alone, none, and the same call twice
        dev = dev_rows(codec, B, lens, shift=3)
        try:
            e = expected(B, lens, idx.set, k, False, pairs=True)
            for path in PATHS:
                codec.set_option(OPTION, path)
                for outputs in ("n", "h", "k", "", "nhk"):
                    out, summ, raw = run(codec, dev, idx, pairs=True, outputs=outputs)
                    assert set(out) == set(outputs)
                    compare(out, summ, e, "outputs %r" % outputs)
                assert run(codec, dev, idx, pairs=True)[1:] == (summ, raw), "the same call on the same context gave other bytes"
        finally:
            codec.set_option(OPTION, None)
            dev.free()
        for n in (0, 1, 2):
            e = check(codec, B[:n], lens[:n], idx, pairs=n != 1, what="n_rows %d" % n)
            assert e["summary"]["n_units"] == (n if n == 1 else n // 2)
        r = codec.screen_rows(0, 0, None, None, idx.ptr, idx.bytes, pairs=True)
        assert summary_of(r) == dict.fromkeys(FIELDS, 0)
    finally:
        idx.free()


# ---------------------------------------------------------------- test 5: the set
def check_set(codec):
    rng = np.random.default_rng(57)
    k = 15
    X, Y, Z = rand_seq(rng, 120), rand_seq(rng, 90), rand_seq(rng, 200)
    withN = Z[:70] + b"N" + Z[71:130] + b"nRY" + Z[133:]
    lists = {"duplicates": [X, Y, X, X], "a sequence and its reverse complement": [X, revcomp(X)], "an N inside": [withN], "lower case": [X.lower(), Y],
             "shorter than k": [X[:14], Y[:3], b"", X[:15]], "none at all": [], "only short ones": [X[:14], b"", Y[:7]], "all": [X, Y.lower(), revcomp(X), withN, b"", X[:14], Y]}
    # rows: the references themselves, the junction of X and Y (its k-mers are in neither), the bytes on either side of the N, strangers
    seqs = [X, Y[:80], revcomp(Y)[:75], X[-30:] + Y[:30], Z[50:100], withN[60:140], rand_seq(rng, 100), X[:14], X[:15]]
    B, lens = rows_of(seqs, 144, "ascii")
    for what, refs in lists.items():
        for option in BUILDS:
            idx = Index(codec, refs, k, option)
            try:
                assert idx.build() == idx.result, "the second build counted otherwise"
                if what == "a sequence and its reverse complement":
                    assert len(idx.set) == len(ref_set([X], k)[0])
                if what in ("none at all", "only short ones"):
                    assert idx.result["n_kmers"] == 0 and idx.result["n_positions"] == 0
                e = check(codec, B, lens, idx, what="the set: %s, built under %s" % (what, option or "default"))
                if what == "all":
                    junction = expected(B[3:4, :60], np.array([60], np.int32), idx.set, k, False)
                    assert junction["hits"][0] == 2 * (30 - k + 1) and junction["kmers"][0] == 60 - k + 1      # (none of the k - 1 k-mers across the junction)
                    assert e["hits"][0] == 120 - k + 1 and e["hits"][6] == 0 and e["hits"][8] == 1
                if not idx.set:
                    assert e["summary"]["hits"] == 0 and e["keep"].all()
            finally:
                idx.free()


def check_placements(codec):
    """a reference of 5,386 bases (S = 16384: the slots fit the LDS) and one of 8,193 (S = 32768: device memory) on the same rows, the index built under default,
    general and collide, screened under default and general: identical outputs, the model's"""
    rng = np.random.default_rng(58)
    k = 25
    big = rand_seq(rng, 8193); refs = {16384: [big[:5386]], 32768: [big]}
    seqs = []
    for i in range(70):
        s = bytearray(rand_seq(rng, 100))
        if i % 4 == 3:                                                        # (R2 of every other pair)
            j = int(rng.integers(0, 8193 - 60)); s[20:80] = big[j:j + 60]
        seqs.append(bytes(s if i % 4 != 3 else revcomp(s)))
    for L in (112, 300):
        B, lens = rows_of(seqs, L, "code", seed=L)
        for S, r in refs.items():
            raws = []
            for option in BUILDS:
                idx = Index(codec, r, k, option)
                try:
                    assert idx.bytes == 64 + 8 * S
                    e = check(codec, B, lens, idx, codes=True, pairs=True, min_hits=3, what="placement S %d built under %s" % (S, option or "default"))
                    assert 0 < e["summary"]["n_matched"] < 35
                    dev = dev_rows(codec, B, lens)
                    try:
                        raws.append(run(codec, dev, idx, codes=True, pairs=True, min_hits=3)[1:])
                    finally:
                        dev.free()
                finally:
                    idx.free()
            assert raws[0] == raws[1] == raws[2], "the index built under another option gave other outputs"


# ---------------------------------------------------------------- test 6: refusals
def _good(codec, idx=None):
    """what every refusal is followed by, on the same context: a build and a screen that give the model's result"""
    rng = np.random.default_rng(9)
    ref = rand_seq(rng, 90)
    own = Index(codec, [ref, ref[:20]], 16)
    try:
        B, lens = rows_of([ref[10:60], rand_seq(rng, 50), revcomp(ref)[:33], ref[:16]], 50, "ascii")
        check(codec, B, lens, own, pairs=True, paths=(None,), what="after a refusal")
        if idx is not None:
            check(codec, B, lens, idx, paths=(None,), what="the caller's index after a refusal")
    finally:
        own.free()


def check_build_refusals(codec):
    from repaq_amd import RfqError
    rng = np.random.default_rng(60)
    refs = [rand_seq(rng, 50), rand_seq(rng, 30), rand_seq(rng, 20)]
    blob = b"".join(refs)
    d_blob = codec.dev_put(blob); buf = W.Guarded(codec, 64 + 8 * 1024 + 64)
    offs = {}

    def off(*v):
        if v not in offs:
            offs[v] = codec.dev_put(np.array(v + (0,), np.uint64).tobytes())
        return offs[v]

    def at(p, k):
        return C.c_void_p(p.value + k)
    good = (0, 50, 80, 100); need = 64 + 8 * 1024
    Bd = codec.screen_build
    try:
        assert int(Bd(d_blob, 100, off(*good), 3, k=16, size_only=True).index_bytes) == need
        calls = ((E_ARG, "k must be", lambda: Bd(d_blob, 100, off(*good), 3, k=3, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "k must be", lambda: Bd(d_blob, 100, off(*good), 3, k=32, size_only=True)),
                 (E_ARG, "null d_refs / d_ref_off", lambda: Bd(None, 100, off(*good), 3, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "null d_refs / d_ref_off", lambda: Bd(d_blob, 100, None, 3, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "8-byte aligned", lambda: Bd(d_blob, 100, at(off(*good), 4), 2, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "16-byte aligned", lambda: Bd(d_blob, 100, off(*good), 3, k=16, d_index=at(buf.ptr, 8), index_cap=need)),
                 (E_ARG, "null d_index", lambda: Bd(d_blob, 100, off(*good), 3, k=16)),
                 (E_ARG, "d_index overlaps the input d_refs", lambda: Bd(d_blob, 100, off(*good), 3, k=16, d_index=at(d_blob, 64), index_cap=need)),
                 (E_NOSPACE, "need %d bytes" % need, lambda: Bd(d_blob, 100, off(*good), 3, k=16, d_index=buf.ptr, index_cap=need - 1)),
                 (E_NOSPACE, "need %d bytes" % need, lambda: Bd(d_blob, 100, off(*good), 3, k=16, d_index=buf.ptr, index_cap=0)),
                 (E_ARG, "first such reference: 1)", lambda: Bd(d_blob, 100, off(0, 50, 40, 100), 3, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "first such reference: 2)", lambda: Bd(d_blob, 100, off(0, 50, 80, 101), 3, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "first such reference: 0)", lambda: Bd(d_blob, 100, off(1 << 40, 50, 80, 100), 3, k=16, d_index=buf.ptr, index_cap=need)),
                 (E_ARG, "first such reference: 0)", lambda: Bd(d_blob, 100, off((1 << 64) - 1, (1 << 64) - 1, 80, 100), 3, k=16, d_index=buf.ptr, index_cap=need)))
        for code, what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == code and what in ei.value.message, (what, ei.value)
            if code == E_NOSPACE:
                assert set(buf.body()) == {0xA5}, "a refused build wrote into the index"
            _good(codec)
        assert buf.guards_intact()
        # no reference at all takes no pointers; an empty set is no error
        r = Bd(None, 0, None, 0, k=16, d_index=buf.ptr, index_cap=need)
        assert summary_of(r, BUILD_FIELDS) == dict(n_refs=0, ref_bases=0, n_positions=0, n_kmers=0, slots=1024, index_bytes=need)
    finally:
        codec.dev_free(d_blob); buf.free()
        for p in offs.values():
            codec.dev_free(p)


def _raw_pairs(codec, rows, idx, pairs):
    """the C call with a `pairs` the Python wrapper cannot express"""
    from repaq_amd import _capi as A
    n, L, pb, pl = rows
    ri = codec._rows_in(n, L, pb, None, pl, None, 0, None, False, 0)
    a = A.ScreenRowsArgs(pairs, 0, 1, 0, idx.ptr, idx.bytes, None, None, None, None); r = A.ScreenRowsResult()
    return codec._L.rfq_screen_rows(codec._h, C.byref(ri), C.byref(a), C.byref(r))


def check_host_refusals(codec):
    from repaq_amd import RfqError
    rng = np.random.default_rng(61)
    idx = Index(codec, [rand_seq(rng, 200)], 16)
    B, lens = rows_of([rand_seq(rng, 30) for _ in range(12)], 32, "ascii")
    n, L = B.shape
    dev = dev_rows(codec, B, lens, np.ones(n, np.uint8))
    buf = codec.dev_put(b"\0" * 16384); b = buf.value
    try:
        rows = dev.adapter_args(); ix = (idx.ptr, idx.bytes)

        def at(p, k):
            return C.c_void_p(p.value + k)
        D = codec.screen_rows
        calls = (("pairs takes rows in pairs", lambda: D(n - 1, L, dev.bases, dev.lens, *ix, pairs=True)),
                 ("pairs must be 0 or 1", lambda: codec._check(_raw_pairs(codec, rows, idx, 2))),
                 ("unknown mode", lambda: D(*rows, *ix, mode=2)),
                 ("unknown mode", lambda: D(*rows, *ix, mode=-1)),
                 ("min_pct must be", lambda: D(*rows, *ix, min_pct=101)),
                 ("bad base_mode", lambda: D(*rows, *ix, base_mode=7)),
                 ("row_len must be >= 1", lambda: D(n, 0, dev.bases, dev.lens, *ix)),
                 ("null d_lens / d_bases", lambda: D(n, L, None, dev.lens, *ix)),
                 ("null d_lens / d_bases", lambda: D(n, L, dev.bases, None, *ix)),
                 ("d_index must be", lambda: D(*rows, None, idx.bytes)),
                 ("d_index must be", lambda: D(*rows, at(idx.ptr, 8), idx.bytes - 8)),
                 ("d_index must be", lambda: D(*rows, idx.ptr, 63)),
                 ("4-byte aligned", lambda: D(n, L, dev.bases, at(dev.lens, 2), *ix)),
                 ("4-byte aligned", lambda: D(*rows, *ix, d_kmers=C.c_void_p(b + 2))),
                 ("4-byte aligned", lambda: D(*rows, *ix, d_hits=C.c_void_p(b + 1))),
                 ("d_keep overlaps the input rows->d_bases", lambda: D(*rows, *ix, d_keep=at(dev.bases, n * L - 1))),
                 ("d_keep overlaps the input d_in", lambda: D(*rows, *ix, d_in=dev.cand, d_keep=dev.cand)),
                 ("d_hits overlaps the input rows->d_lens", lambda: D(*rows, *ix, d_hits=dev.lens)),
                 ("d_kmers overlaps the input d_index", lambda: D(*rows, *ix, d_kmers=at(idx.ptr, idx.bytes - 4))),
                 ("d_keep overlaps the input d_index", lambda: D(*rows, *ix, d_keep=idx.ptr)),
                 ("too many rows", lambda: D(1 << 31, 1, dev.bases, dev.lens, *ix)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == E_ARG and what in ei.value.message, (what, ei.value)
            _good(codec, idx)
        # (outputs of the caller's own that lie on nothing are taken; the quality rows are not an input; no rows at all are no error)
        assert D(*rows, *ix, d_kmers=C.c_void_p(b), d_hits=C.c_void_p(b + 1024), d_keep=C.c_void_p(b + 4096)).n_units == n
        assert summary_of(D(0, 0, None, None, *ix, pairs=True)) == dict.fromkeys(FIELDS, 0)
    finally:
        dev.free(); codec.dev_free(buf); idx.free()


def check_bad_index(codec):
    """RFQ_E_DATA for a header rfq_screen_build does not write; an index whose slots are ALL non-empty, written by the test: the call returns, the walk is bounded"""
    from repaq_amd import RfqError
    rng = np.random.default_rng(62)
    ref = rand_seq(rng, 100); k = 16
    idx = Index(codec, [ref], k)
    B, lens = rows_of([ref[:60], rand_seq(rng, 60), ref[40:]], 64, "ascii")
    dev = dev_rows(codec, B, lens)
    copies = []
    try:
        img = bytearray(idx.g.body())
        hdr = np.frombuffer(bytes(img[:64]), np.uint32).copy()               # magic (2 words), version, k, S (2 words), n_kmers (2 words), flags
        assert hdr[3] == k and hdr[4] == 1024 and hdr[5] == 0 and hdr[6] == len(idx.set)

        def variant(**words):
            h = hdr.copy()
            for w, v in words.items():
                h[int(w[1:])] = v
            p = codec.dev_put(h.tobytes() + bytes(img[64:])); copies.append(p)
            return p
        for what, words in (("does not begin with the header", dict(w0=int(hdr[0]) ^ 1)), ("does not begin with the header", dict(w2=2)), ("the index's k", dict(w3=0)),
                            ("the index's k", dict(w3=32)), ("slot count", dict(w4=1000)), ("slot count", dict(w4=0)), ("slot count", dict(w4=2048)),
                            ("slot count", dict(w5=1))):
            with R.pytest_raises(RfqError) as ei:
                run(codec, dev, idx, index=(variant(**words), idx.bytes))
            assert ei.value.code == E_DATA and what in ei.value.message, (what, words, ei.value)
            _good(codec, idx)
        # a copy of the good index is as good as the index
        e = expected(B, lens, idx.set, k, False)
        out, summ, _ = run(codec, dev, idx, index=(variant(), idx.bytes))
        compare(out, summ, e, "a copy of the index:")
        # every slot taken, none of them by a k-mer of these rows (the values are above 4^16): every probe walks all S slots and misses
        full = (np.arange(1024, dtype=np.uint64) + np.uint64(1 << 40)) | np.uint64(1 << 63)
        p = codec.dev_put(hdr.tobytes() + full.tobytes()); copies.append(p)
        for path in PATHS:
            codec.set_option(OPTION, path)
            out, summ, _ = run(codec, dev, idx, index=(p, idx.bytes))
            compare(out, summ, expected(B, lens, set(), k, False), "a full index, %s:" % (path or "default"))
        codec.set_option(OPTION, None)
        _good(codec, idx)
        # headers that pass every check with FEWER slots than the build ever makes, with the collide flag (its start slot is four bits of the value: it has to be
        # masked like the hash) and without, the buffer ending with its S slots: the slots hold k-mers of the first row, and exactly those hit
        vals = sorted(set(kmers_of(digits(ref[:60], False), k)))
        for S in (1, 2, 4, 8, 16):
            for flags in (1, 0):
                h = hdr.copy(); h[4] = S; h[8] = flags
                tab = (np.array(vals[5:5 + S], np.uint64)[::-1]) | np.uint64(1 << 63)
                p = codec.dev_put(h.tobytes() + tab.tobytes()); copies.append(p)
                for path in PATHS:
                    codec.set_option(OPTION, path)
                    out, summ, _ = run(codec, dev, idx, index=(p, 64 + 8 * S))
                    compare(out, summ, expected(B, lens, set(vals[5:5 + S]), k, False), "S %d flags %d, %s:" % (S, flags, path or "default"))
                    assert summ["hits"] >= S
                codec.set_option(OPTION, None)
        _good(codec, idx)
    finally:
        codec.set_option(OPTION, None)
        dev.free(); idx.free()
        for p in copies:
            codec.dev_free(p)


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "last", "pair_r1", "pair_r2")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    rng = np.random.default_rng(63)
    small, large = Index(codec, [rand_seq(rng, 100)], 15), Index(codec, [rand_seq(rng, 8200)], 15)
    try:
        for L, n in ((24, 300), (300, 10), (1100, 6)):
            B = np.frombuffer(rand_seq(rng, n * L), np.uint8).reshape(n, L); lens = rng.integers(0, L + 1, n).astype(np.int32)
            pairs = where.startswith("pair")
            row = dict(first=0, last=n - 1, pair_r1=n // 2 & ~1, pair_r2=(n // 2 & ~1) + 1)[where]
            lens[row] = -1 if value == "negative" else L + 1
            for cand in (None, (np.arange(n) != row).astype(np.uint8)):      # (every row is judged, candidate or not)
                dev = dev_rows(codec, B, lens, cand, shift=1)
                try:
                    for idx in (small, large):
                        for path in PATHS:
                            codec.set_option(OPTION, path)
                            for outputs in ("", "nhk"):
                                with R.pytest_raises(RfqError) as ei:
                                    run(codec, dev, idx, pairs=pairs, outputs=outputs)
                                assert ei.value.code == E_ARG and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                            codec.set_option(OPTION, None)
                    _good(codec, small)
                finally:
                    codec.set_option(OPTION, None)
                    dev.free()
        # two bad rows: the first is named
        lens = np.full(n, L, np.int32); lens[1] = -5; lens[4] = L + 1
        dev = dev_rows(codec, B, lens)
        try:
            with R.pytest_raises(RfqError) as ei:
                run(codec, dev, small)
            assert "first such row: 1)" in ei.value.message
        finally:
            dev.free()
        _good(codec, small)
    finally:
        small.free(); large.free()


def check_option(codec, reset):
    from repaq_amd import RfqError
    assert OPTION in codec.option_names() and codec.get_option(OPTION) == ""
    for v in ("collide", "general"):
        codec.set_option(OPTION, v)
        assert codec.get_option(OPTION) == v
        reset(codec)
        assert codec.get_option(OPTION) == ""
    for bad in ("staged", "Collide", "1"):
        with R.pytest_raises(RfqError):
            codec.set_option(OPTION, bad)
    assert codec.get_option(OPTION) == ""


# ---------------------------------------------------------------- test 7: state and composition
def check_state(codec):
    """a screen (build and rows) between two rfq_dedup_rows calls and two rfq_rows_to_text calls on one context leaves their results byte-identical"""
    import _dedup as D
    from repaq_amd import PE_TWO_FILES
    B, Q, lens = D.planted(40, True, 64, sizes=(30, 7, 2) + (1,) * 20)
    n = len(lens)
    names = [b"@r%d" % i for i in range(n)]
    dd = D.dev_rows(codec, B, Q, lens); dt = W.DevRows(codec, B & 3, Q % 40, np.maximum(lens, 1), names)
    try:
        def calls():
            d = D.run(codec, dd, pairs=True, best=True, hist_len=8)
            r = codec.rows_to_text(*dt.args(), paired=PE_TWO_FILES, codes=True, qual_offset=33)
            return d[1], d[2], codec.dev_get(r.d_fq1, r.n1), codec.dev_get(r.d_fq2, r.n2)
        first = calls()
        _good(codec)
        rng = np.random.default_rng(65)
        idx = Index(codec, [rand_seq(rng, 9000)], 21)
        try:
            Bs, ls = rows_of([rand_seq(rng, 300) for _ in range(9)], 300, "ascii")
            check(codec, Bs, ls, idx, what="between the calls")
        finally:
            idx.free()
        assert calls() == first, "a screen between them changed what rfq_dedup_rows or rfq_rows_to_text give"
    finally:
        dd.free(); dt.free()


COMPOSE_K = 21


def compose_text(pairs=240, seed=14):
    """_adapter.compose_text's records (fragments of 40 .. 400 bases with the adapters behind them) where every fourth fragment comes from a contaminant of 700
    bases and every sixth pair comes again further on, under a name of its own; returns (the two lists of records, the contaminant)"""
    import _adapter as A
    rng = np.random.default_rng(seed)
    contaminant = rand_seq(rng, 700)
    a = (A.AD1 + b"ACGTTGCATTGACCA" * 12, A.AD2 + b"TTGACGGATCAGGCA" * 12)
    recs = []
    for i in range(pairs):
        ins = int(rng.integers(40, 401))
        if i % 4 == 1:
            j = int(rng.integers(0, 700 - ins)); f = contaminant[j:j + ins]
            f = revcomp(f) if i % 8 == 1 else f
        else:
            f = rand_seq(rng, ins)
        pair = []
        for m, fr in ((0, f), (1, revcomp(f))):
            s = (fr + a[m])[:150]
            q = np.clip(38 - np.arange(150) * int(rng.integers(0, 30)) // 150 + rng.integers(-4, 5, 150), 2, 41).astype(np.uint8)
            pair.append((s, bytes(q + 33)))
        recs.append(pair)
    order = rng.permutation(np.concatenate([np.arange(pairs), np.arange(0, pairs, 6)]))
    out = [[], []]
    for x, i in enumerate(order):
        for m in (0, 1):
            out[m].append(b"@frag.%d %d/%d\n" % (x + 1, i, m + 1) + recs[i][m][0] + b"\n+\n" + recs[i][m][1] + b"\n")
    return out, contaminant


def compose_expected(t1, t2, ca, cj, contaminant):
    """the two texts adapter removal, the judge on the shortened reads, the screen of the judge's pairs against the contaminant, dedup of what the screen left and
    the pair rule leave; the screen and dedup look at the reads as the adapter step cut them, the texts hold the judge's windows"""
    import _adapter as A
    import _judge as J
    rows = [rec.split(b"\n")[:4] for pair in zip(t1, t2) for rec in pair]
    L = max(len(r[1]) for r in rows)
    B = np.zeros((len(rows), L), np.uint8); lens = np.array([len(r[1]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        B[i, :len(r[1])] = np.frombuffer(r[1], np.uint8)
    cut = A.expected(B, lens, ca, False)["length"]
    S = ref_set([contaminant], COMPOSE_K)[0]
    seen = set(); out = [[], []]; counts = dict(judged=0, matched=0, dups=0)
    for i in range(0, len(rows), 2):
        v = []
        for g in (i, i + 1):
            name, s, _, q = rows[g]
            k, a, m, _, _ = J.judge_row(list(s), [x - 33 for x in q], int(cut[g]), cj, False)
            v.append((k and m >= cj["min_len"], name, s[:int(cut[g])], s[a:a + m], q[a:a + m]))
        if not (v[0][0] and v[1][0]):
            continue
        counts["judged"] += 1
        if any(x in S for w in v for x in kmers_of(digits(w[2], False), COMPOSE_K)):
            counts["matched"] += 1
            continue
        key = (v[0][2], v[1][2])
        if key in seen:
            counts["dups"] += 1
            continue
        seen.add(key)
        for m in (0, 1):
            out[m].append(v[m][1] + b"\n" + v[m][3] + b"\n+\n" + v[m][4] + b"\n")
    return b"".join(out[0]), b"".join(out[1]), len(out[0]), counts


def compose_criteria():
    import _adapter as A
    import _judge as J
    return A.COMPOSE_A, J.crit(cut_flags=J.TAIL, cut_window=4, cut_mean_q=20, min_len=30, min_mean_q=20)


def check_composition(codec):
    """text -> adapter -> judge -> screen (the judge's mask) -> dedup (the screen's mask) -> select -> text equals the host's text"""
    from repaq_amd import PE_TWO_FILES
    (t1, t2), contaminant = compose_text()
    ca, cj = compose_criteria()
    w1, w2, kept, counts = compose_expected(t1, t2, ca, cj, contaminant)
    assert kept > 50 and counts["matched"] > 20 and counts["dups"] > 10, (kept, counts)
    _, B, Q, lens, names = codec.text_rows_bytes(b"".join(t1), b"".join(t2), paired=PE_TWO_FILES, row_len=160, qual_offset=33)
    n = len(lens)
    dev = W.DevRows(codec, B, Q, lens, names)
    idx = Index(codec, [contaminant], COMPOSE_K)
    ga, gk, gs, gl, gc, gd = (W.Guarded(codec, k) for k in (4 * n, n, 4 * n, 4 * n, n, n))
    bufs = []
    try:
        codec.adapter_rows(n, 160, dev.bases, dev.lens, d_len=ga.ptr, **ca)
        codec.judge_rows(n, 160, dev.bases, dev.quals, ga.ptr, **cj, d_keep=gk.ptr, d_start=gs.ptr, d_len=gl.ptr)
        c = codec.screen_rows(n, 160, dev.bases, ga.ptr, idx.ptr, idx.bytes, pairs=True, d_in=gk.ptr, d_keep=gc.ptr)
        d = codec.dedup_rows(n, 160, dev.bases, dev.quals, ga.ptr, pairs=True, d_in=gc.ptr, d_keep=gd.ptr)
        assert all(g.guards_intact() for g in (ga, gk, gs, gl, gc, gd))
        assert (int(c.n_candidates), int(c.n_matched), int(d.n_candidates), int(d.n_dups)) == (counts["judged"], counts["matched"], counts["judged"] - counts["matched"], counts["dups"])
        sel = dict(d_keep=gd.ptr, d_start=gs.ptr, d_len=gl.ptr, pairs=True, min_len=cj["min_len"])
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
        dev.free(); idx.free()
        for g in (ga, gk, gs, gl, gc, gd):
            g.free()
        for p in bufs:
            codec.dev_free(p)


# ---------------------------------------------------------------- test 9: more units than one step of the LDS placement's capped grid takes
def check_many_rows(codec, n=200_006):
    """Short rows, many more than a step of the LDS placement's grid of one or two workgroups per compute unit holds (64 units a workgroup and step at this row
    length), so that a workgroup takes several steps and the last one is part empty; against an index of 2048 slots (two workgroups a compute unit) and one of 16384
    (one).  The rows are 997 distinct ones in a fixed order: the model judges those, the verdict and the sums are formed over all rows from its counts."""
    rng = np.random.default_rng(67)
    k, L, D = 15, 48, 997
    ref = rand_seq(rng, 5386)
    seqs = []
    for i in range(D):
        s = bytearray(rand_seq(rng, int(rng.integers(0, L + 1))))
        if i % 3 == 0 and len(s) >= 30:
            j = int(rng.integers(0, 5300)); s[5:5 + 22] = ref[j:j + 22]
        seqs.append(bytes(s))
    Bd, ld = rows_of(seqs, L, "code")
    pick = (np.arange(n, dtype=np.int64) * 7 + np.arange(n, dtype=np.int64) // D) % D
    B, lens = np.ascontiguousarray(Bd[pick]), ld[pick]
    for refs in ([ref[:900]], [ref]):
        idx = Index(codec, refs, k)
        try:
            d = expected(Bd, ld, idx.set, k, True)
            kmers, hits = d["kmers"][pick], d["hits"][pick]
            dev = dev_rows(codec, B, lens)
            try:
                for pairs in (False, True):
                    nr = 2 if pairs else 1
                    K = kmers.astype(np.int64).reshape(-1, nr).sum(1); H = hits.astype(np.int64).reshape(-1, nr).sum(1); bases = lens.astype(np.int64).reshape(-1, nr).sum(1)
                    matched = (H >= 2) & (100 * H >= 10 * K)
                    e = dict(kmers=kmers, hits=hits, keep=np.repeat(~matched, nr).astype(np.uint8),
                             summary=dict(n_units=n // nr, n_candidates=n // nr, n_matched=int(matched.sum()), n_kept=int((~matched).sum()), kmers=int(K.sum()), hits=int(H.sum()),
                                          bases_in=int(bases.sum()), bases_kept=int(bases[~matched].sum())))
                    assert 0 < e["summary"]["n_matched"] < n // nr
                    out, summ, _ = run(codec, dev, idx, codes=True, pairs=pairs, min_hits=2, min_pct=10)
                    compare(out, summ, e, "many rows, %d slots, pairs %d:" % ((idx.bytes - 64) // 8, pairs))
            finally:
                dev.free()
        finally:
            idx.free()
