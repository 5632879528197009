"""Shared helpers of the rfq_kmers_init / rfq_kmers_rows / rfq_kmers_read tests (tests/test_emu_kmers.py on the SIMT interpreter, tests/test_gpu_kmers.py on the
MI355X).

Nothing expected comes from the code under test: the model is a collections.Counter of canonical ints made by a plain loop over the positions of every counted
row (the k-mer helpers of tests/_screen.py: a k-mer is a string of base-4 digits, its value int(s, 4)), the spectrum a loop over the Counter's values.  Every
comparison is exact integer equality.  A table is compared through rfq_kmers_read: the selected (value, count) pairs as a sorted list against the model's, d_hist
against the model's spectrum, the header's n_kmers and total against the model's.  Every call runs in _rows.Guarded buffers of exactly the bytes it may write - the
table included - and the guards are checked after each call."""
import collections
import ctypes as C
import re

import numpy as np

import _rows as W
import _rows_enc as R
import _screen as S

ROWS_FIELDS = ("n_rows", "n_counted", "bases_in", "added", "n_new", "n_kmers", "total", "lost")
READ_FIELDS = ("k", "slots", "n_kmers", "total", "max_count", "n_selected", "selected_total", "index_slots", "index_bytes")
OPTION = "RFQ_KMERS"
PATHS = (None, "general", "direct")
FORMS = (None, "general", "direct", "collide")
E_ARG, E_DATA, E_NOSPACE = S.E_ARG, S.E_DATA, S.E_NOSPACE
KM_ITER = 4                                                                    # (enc/rows_kmers.h)


# ---------------------------------------------------------------- the model
def pow2(want):
    s = 1024
    while s < want:
        s *= 2
    return s


def model(B, lens, k, codes, cand=None):
    """(Counter of canonical values, kmers [n] uint32, summary without the table's state) of the counted rows; a row's k-mers are formed once per distinct row"""
    n = len(lens); cnt = collections.Counter(); kmers = np.zeros(n, np.uint32); seen = {}
    s = dict(n_rows=n, n_counted=0, bases_in=0, added=0)
    Bb = [bytes(r) for r in np.ascontiguousarray(B)]
    for g in range(n):
        if cand is not None and not int(cand[g]):
            continue
        key = Bb[g][:int(lens[g])]
        if key not in seen:
            seen[key] = collections.Counter(S.kmers_of(S.digits(key, codes), k))
        c = seen[key]
        cnt.update(c); kmers[g] = sum(c.values())
        s["n_counted"] += 1; s["bases_in"] += int(lens[g]); s["added"] += int(kmers[g])
    return cnt, kmers, s


def spectrum(cnt, hist_len):
    h = np.zeros(hist_len, np.uint64)
    for c in cnt.values() if hist_len else ():
        h[min(c, hist_len) - 1] += 1
    return h


def selected(cnt, min_count=1, max_count=0):
    return sorted((v, c) for v, c in cnt.items() if c >= max(min_count, 1) and (max_count == 0 or c <= max_count))


def summary_of(r, fields):
    return {f: int(getattr(r, f)) for f in fields}


# ---------------------------------------------------------------- the calls
class Table:
    """a table formatted by rfq_kmers_init in a Guarded buffer of exactly table_bytes, beside the model's Counter of everything counted into it so far.
    option: the value of RFQ_KMERS the table is formatted under"""
    def __init__(self, codec, k, slots, option=None):
        self.codec, self.k, self.cnt, self.g = codec, k, collections.Counter(), None
        codec.set_option(OPTION, option)
        try:
            q = codec.kmers_init(k=k, slots=slots, size_only=True)
            want = pow2(slots)
            assert (int(q.slots), int(q.table_bytes)) == (want, 64 + 16 * want), (int(q.slots), int(q.table_bytes), want)
            self.S, self.bytes = want, int(q.table_bytes)
            self.g = W.Guarded(codec, self.bytes)
            self.init()
        except Exception:
            self.free()
            raise
        finally:
            codec.set_option(OPTION, None)

    def init(self):
        r = self.codec.kmers_init(k=self.k, slots=self.S, d_table=self.g.ptr, table_cap=self.bytes)
        assert self.g.guards_intact(), "a guard around the table was written"
        assert (int(r.slots), int(r.table_bytes)) == (self.S, self.bytes)
        self.cnt = collections.Counter()

    @property
    def ptr(self):
        return self.g.ptr

    def free(self):
        if self.g is not None:
            self.g.free()

    def count(self, dev, codes=False, want_kmers=True, table=None):
        """one rfq_kmers_rows; returns (d_kmers as numpy or None, summary, raw bytes of d_kmers)"""
        codec = self.codec
        gk = W.Guarded(codec, 4 * dev.n) if want_kmers else None
        ptr, nbytes = table if table is not None else (self.ptr, self.bytes)
        try:
            r = codec.kmers_rows(*dev.adapter_args(), ptr, nbytes, codes=codes, d_in=dev.cand, d_kmers=gk.ptr if gk else None)
            assert self.g.guards_intact() and (gk is None or gk.guards_intact()), "a guard around the table or d_kmers was written"
            raw = gk.body() if gk else b""
            return (np.frombuffer(raw, np.uint32) if gk else None), summary_of(r, ROWS_FIELDS), raw
        finally:
            if gk:
                gk.free()

    def add(self, B, lens, codes=False, cand=None, shift=0, option=None, what=""):
        """rows into the table under `option`, the call's outputs and result against the model's; returns the model's kmers"""
        codec = self.codec
        c, kmers, s = model(B, lens, self.k, codes, cand)
        n_new = len(set(c) - set(self.cnt))
        self.cnt.update(c)
        want = dict(s, n_new=n_new, n_kmers=len(self.cnt), total=sum(self.cnt.values()), lost=0)
        dev = S.dev_rows(codec, B, lens, cand, shift)
        try:
            codec.set_option(OPTION, option)
            got, summ, _ = self.count(dev, codes)
        finally:
            codec.set_option(OPTION, None)
            dev.free()
        if not np.array_equal(got, kmers):
            bad = np.nonzero(got != kmers)[0]
            raise AssertionError("%s kmers differ in %d of %d rows, first %d: got %r, want %r" % (what, len(bad), len(kmers), bad[0], got[bad[0]], kmers[bad[0]]))
        assert summ == want, (what, option, {f: (summ[f], want[f]) for f in ROWS_FIELDS if summ[f] != want[f]})
        return kmers

    def read(self, min_count=1, max_count=0, hist_len=0, index=False, table=None):
        """rfq_kmers_read: a size query, then Guarded buffers of exactly n_selected entries / hist_len bins / index_bytes; returns dict(pairs sorted, hist,
        summary, index: the Guarded buffer - the caller frees it - or None)"""
        codec = self.codec
        ptr, nbytes = table if table is not None else (self.ptr, self.bytes)
        q = codec.kmers_read(ptr, nbytes, min_count=min_count, max_count=max_count, size_only=True, hist_len=hist_len)
        ns, ib = int(q.n_selected), int(q.index_bytes)
        assert int(q.index_slots) == pow2(2 * ns) and ib == 64 + 8 * int(q.index_slots)
        gv, gc, gh = W.Guarded(codec, 8 * ns), W.Guarded(codec, 8 * ns), W.Guarded(codec, 8 * hist_len)
        gi = W.Guarded(codec, ib) if index else None
        try:
            r = codec.kmers_read(ptr, nbytes, min_count=min_count, max_count=max_count, hist_len=hist_len, d_hist=gh.ptr if hist_len else None, d_values=gv.ptr,
                                 d_counts=gc.ptr, list_cap=ns, d_index=gi.ptr if gi else None, index_cap=ib if gi else 0)
            assert all(x.guards_intact() for x in (gv, gc, gh, self.g) + ((gi,) if gi else ())), "a guard around an output of the read was written"
            assert summary_of(r, READ_FIELDS) == summary_of(q, READ_FIELDS), "the size query and the read report differently"
            vals = np.frombuffer(gv.body(), np.uint64); cnts = np.frombuffer(gc.body(), np.uint64)
            return dict(pairs=sorted(zip(vals.tolist(), cnts.tolist())), hist=np.frombuffer(gh.body(), np.uint64).copy(), summary=summary_of(r, READ_FIELDS), index=gi)
        except Exception:
            if gi:
                gi.free()
            raise
        finally:
            for x in (gv, gc, gh):
                x.free()

    def check(self, hist_len=16, min_count=1, max_count=0, cnt=None, what=""):
        """the table equals the model: the selected pairs, the spectrum, the header's counts"""
        cnt = self.cnt if cnt is None else cnt
        got = self.read(min_count, max_count, hist_len)
        want = selected(cnt, min_count, max_count)
        assert got["pairs"] == want, "%s: the selected pairs differ: %d against the model's %d, first %r" % (
            what, len(got["pairs"]), len(want), next((x for x in zip(got["pairs"], want) if x[0] != x[1]), None))
        assert np.array_equal(got["hist"], spectrum(cnt, hist_len)), (what, got["hist"].tolist(), spectrum(cnt, hist_len).tolist())
        s = got["summary"]
        w = dict(k=self.k, slots=self.S, n_kmers=len(cnt), total=sum(cnt.values()), max_count=max(cnt.values(), default=0), n_selected=len(want),
                 selected_total=sum(c for _, c in want), index_slots=pow2(2 * len(want)), index_bytes=64 + 8 * pow2(2 * len(want)))
        assert s == w, (what, {f: (s[f], w[f]) for f in READ_FIELDS if s[f] != w[f]})
        hdr = np.frombuffer(self.g.body()[:64], np.uint64)                    # magic, version | k << 32, S, n_kmers, total, flags
        assert (int(hdr[1]) >> 32, int(hdr[2]), int(hdr[3]), int(hdr[4])) == (self.k, self.S, len(cnt), sum(cnt.values())), (what, hdr.tolist())
        return got


def counted(codec, B, lens, k, codes=False, cand=None, shifts=(0,), paths=PATHS, slots=None, what=""):
    """the rows into a fresh table at every shift and under every path: each table equals the model; returns the model's Counter"""
    cnt = None
    for shift in shifts:
        for path in paths:
            t = Table(codec, k, slots if slots is not None else 2 * sum(max(int(l) - k + 1, 0) for l in lens), "collide" if path == "collide" else None)
            try:
                t.add(B, lens, codes, cand, shift, None if path == "collide" else path, "%s shift %d option %s:" % (what, shift, path or "default"))
                t.check(what="%s shift %d option %s" % (what, shift, path or "default"))
                cnt = t.cnt
            finally:
                t.free()
    return cnt


# ---------------------------------------------------------------- test 1: every position, every k
KS = (4, 5, 15, 16, 17, 31)


def check_every_position(codec, k):
    """a planted k-mer at every start 0 .. 48 - k of a 48-base row, in ASCII, lower case and codes, and the same rows reverse-complemented: table = model (the
    reverse complements give the SAME table), kmers = l - k + 1"""
    ref = S.apart_reference(k, k)
    seqs = [S.BACKGROUND]
    for s in range(48 - k + 1):
        j = s % 41
        seqs.append(S.BACKGROUND[:s] + ref[j:j + k] + S.BACKGROUND[s + k:])
    tables = []
    for mode in S.MODES:
        for rows in (seqs, [S.revcomp(x) for x in seqs]):
            B, lens = S.rows_of(rows, 48, mode)
            cnt = counted(codec, B, lens, k, codes=mode == "code", shifts=(0, 5), paths=(None, "general"), what="k %d %s" % (k, mode))
            _, kmers, _ = model(B, lens, k, mode == "code")
            assert (kmers == 48 - k + 1).all()
            tables.append(cnt)
    assert all(t == tables[0] for t in tables), "the three forms and the reverse complements of the same rows count otherwise"
    for s in range(48 - k + 1):
        assert tables[0][S.canon(S.digits(ref[s % 41:s % 41 + k], False))] >= 1


# ---------------------------------------------------------------- test 2: validity
def check_validity(codec):
    rng = np.random.default_rng(72)
    for k, mode in ((4, "ascii"), (16, "code"), (17, "lower"), (31, "ascii")):
        codes = mode == "code"
        ref = S.rand_seq(rng, 48)
        seqs = [ref] + [ref[:p] + b"N" + ref[p + 1:] for p in range(48)]
        B, lens = S.rows_of(seqs, 48, mode)
        if codes:
            for p in range(0, 48, 3):
                B[1 + p, p] = (4, 5, 255)[p % 3]                             # (any code above 3)
        counted(codec, B, lens, k, codes=codes, what="an other byte, k %d" % k)
        _, kmers, _ = model(B, lens, k, codes)
        full = 48 - k + 1
        for p in range(48):
            covered = min(p, full - 1) - max(p - k + 1, 0) + 1
            assert kmers[1 + p] == full - covered, (k, p, kmers[1 + p])
        # l = 0, 1, k - 1, k, k + 1 - the bytes behind the read are the reference's own: never counted
        B = np.tile(np.frombuffer(S.as_mode(ref, mode), np.uint8), (6, 1)); lens = np.array([0, 1, k - 1, k, k + 1, 48], np.int32)
        cnt = counted(codec, B, lens, k, codes=codes, shifts=(0, 1), what="short rows, k %d" % k)
        assert sum(cnt.values()) == 0 + 0 + 0 + 1 + 2 + full
    own = b"ACGT" * 4
    assert S.revcomp(own) == own
    B, lens = S.rows_of([b"TTTTT" + own + b"GGGGGGG", own, own + own], 32, "ascii")
    cnt = counted(codec, B, lens, 16, what="self-complementary")
    v = S.canon(S.digits(own, False))
    assert cnt[v] == 1 + 1 + 5, "a k-mer that is its own reverse complement counts once per occurrence"     # (ACGT x 8 holds it at 0, 4, 8, 12, 16)


# ---------------------------------------------------------------- test 3: seams
def seam_rows(label, seed=73):
    """rows of the seam length `label` (tests/_screen.SEAM_LENS), random - the model counts EVERY position's k-mer, so every lane, kernel and tile seam is judged
    by every row - with k-mers of a reference across 16-byte lane boundaries as _screen.check_seams plants them (repeated values next to the seams, and around every
    plant k-mers that share their last bases and differ in front of them: what sc_start alone would send to one slot), a few of them shorter; returns (k, L, seqs, lens)"""
    k = 31 if label in ("1024", "2049+k") else (4 if label in ("15", "16", "17") else 17)
    L = 2049 + k if label == "2049+k" else int(label)
    rng = np.random.default_rng(seed + L)
    ref = S.rand_seq(rng, k + 40)
    seqs = []
    for phase in (1, 0, 2):
        for r in range(0, k + 1, 1 if L < 1000 else 3):
            s = bytearray(S.rand_seq(rng, L))
            for b in range(16, L + 16, 16):
                at = b - r
                if 0 <= at and at + k <= L and (b // 16) % 3 == phase:
                    j = (b // 16 + r) % 41
                    s[at:at + k] = ref[j:j + k]
            seqs.append(bytes(s))
    lens = np.full(len(seqs), L, np.int32)
    lens[1::5] = rng.integers(0, L + 1, len(lens[1::5]))
    return k, L, seqs, lens


def check_seams(codec, label, paths=PATHS):
    k, L, seqs, lens = seam_rows(label)
    for mode, shifts in (("ascii", (0, 3)), ("code", (9,))):
        B, _ = S.rows_of(seqs, L, mode)
        cnt = counted(codec, B, lens, k, codes=mode == "code", shifts=shifts, paths=paths, what="seams L %d %s" % (L, mode))
        assert max(cnt.values()) > 1 and len(cnt) > 1


def check_walk(codec, label):
    """row counts around a wave, a step and a workgroup of the common path (256 threads, KM_ITER steps): a last partial workgroup, more rows than one step"""
    L, path, counts = W.walk_case(label, KM_ITER)
    rng = np.random.default_rng(74 + L)
    k = 15
    ref = S.rand_seq(rng, 600)
    for n in counts:
        seqs = []
        for i in range(n):
            l = int(rng.integers(0, 41)) if i % 4 else 40
            s = bytearray(S.rand_seq(rng, l))
            if i % 3 == 0 and l >= 20:
                j = int(rng.integers(0, 580)); s[3:3 + 17] = ref[j:j + 17]
            seqs.append(bytes(s))
        B, lens = S.rows_of(seqs, L, "ascii", pad=ord("A"))
        B[:, L - 16:] = np.frombuffer(ref[:16], np.uint8)                     # (the row's last lane holds bytes, none of them inside a read)
        cand = (np.arange(n) % 7 != 3).astype(np.uint8) if n > 8 else None
        counted(codec, B, lens, k, cand=cand, shifts=(n % 16,), paths=(path,) if path else (None, "direct"), what="walk L %d rows %d" % (L, n))


def check_walk_bad_length(codec):
    """a bad length in the last row, a workgroup's first row behind its last step: the refusal names it"""
    from repaq_amd import RfqError
    rng = np.random.default_rng(75)
    t = Table(codec, 15, 4096)
    try:
        for L in (256, 272):
            n = 256 // (16 if L <= 256 else 64) * KM_ITER + 1
            B, lens = S.rows_of([S.rand_seq(rng, 30)] * n, L)
            lens[n - 1] = L + 1
            dev = S.dev_rows(codec, B, lens)
            try:
                with R.pytest_raises(RfqError) as ei:
                    t.count(dev)
                assert ei.value.code == E_ARG and "first such row: %d)" % (n - 1) in ei.value.message, (L, ei.value)
            finally:
                dev.free()
    finally:
        t.free()


# ---------------------------------------------------------------- test 4: adding up
def check_adding_up(codec):
    import _adapter as A
    rng = np.random.default_rng(76)
    k = 17
    shared = S.rand_seq(rng, 300)
    def rows(n, seed):
        r = np.random.default_rng(seed); out = []
        for i in range(n):
            s = bytearray(S.rand_seq(r, int(r.integers(0, 101))))
            if i % 2 == 0 and len(s) >= 40:
                j = int(r.integers(0, 260)); s[2:38] = shared[j:j + 36]
            out.append(bytes(s))
        return out
    a, b = rows(70, 1), rows(50, 2)
    Ba, la = S.rows_of(a, 112, "ascii"); Bb, lb = S.rows_of(b, 112, "ascii"); Bab, lab = S.rows_of(a + b, 112, "ascii")
    ca, cb = model(Ba, la, k, False)[0], model(Bb, lb, k, False)[0]
    reads = []
    for order in ("ab", "ba", "a+b"):
        for path in PATHS:
            t = Table(codec, k, 2 * (len(ca) + len(cb)))
            try:
                if order == "a+b":
                    t.add(Bab, lab, option=path, what="A + B in one call")
                else:
                    for x in order:                                          # (Table.add compares n_new with the values the table did not hold before the call)
                        t.add(*((Ba, la) if x == "a" else (Bb, lb)), option=path, what="order %s, rows %s" % (order, x))
                assert t.cnt == ca + cb
                reads.append(t.check(hist_len=8, what="order %s under %s" % (order, path or "default")))
            finally:
                t.free()
    assert all(r["pairs"] == reads[0]["pairs"] and np.array_equal(r["hist"], reads[0]["hist"]) and r["summary"] == reads[0]["summary"] for r in reads)
    assert len(set(cb) - set(ca)) > 0 and len(set(cb) & set(ca)) > 0          # (the second call's n_new is neither 0 nor all of its values)
    # d_in masks rows out (any non-zero byte counts a row); d_kmers equals rfq_screen_rows' d_kmers on the same rows and mask
    cand = np.array([(0, 1, 7, 255)[i % 4] for i in range(len(la))], np.uint8)
    idx = S.Index(codec, [shared], k)
    t = Table(codec, k, 2 * len(ca))
    try:
        t.add(Ba, la, cand=cand, shift=3, what="a mask")
        t.check(what="a mask")
        assert t.cnt != ca and sum(t.cnt.values()) > 0
        for cd in (cand, None):
            dev = S.dev_rows(codec, Ba, la, cd, 1)
            try:
                t.init()
                _, _, raw = t.count(dev)
                out, _, sraw = S.run(codec, dev, idx, outputs="n")
                assert raw == sraw["n"], "d_kmers differs from rfq_screen_rows' d_kmers"
            finally:
                dev.free()
    finally:
        t.free(); idx.free()
    # lens cut by rfq_adapter_rows are honoured
    ad = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
    seqs = [S.rand_seq(rng, int(rng.integers(30, 90))) + ad for _ in range(24)] + [S.rand_seq(rng, 100) for _ in range(8)]
    B, lens = S.rows_of([s[:112] for s in seqs], 112, "ascii")
    dev = S.dev_rows(codec, B, lens)
    gl = W.Guarded(codec, 4 * len(lens))
    t = Table(codec, k, 8192)
    try:
        codec.adapter_rows(len(lens), 112, dev.bases, dev.lens, d_len=gl.ptr, adapter1=ad, adapter_min=8)
        cut = np.frombuffer(gl.body(), np.int32)
        assert (cut[:24] < lens[:24]).all() and (cut[24:] == lens[24:]).all(), "the adapter step did not cut the planted adapters"
        r = codec.kmers_rows(len(lens), 112, dev.bases, gl.ptr, t.ptr, t.bytes)
        t.cnt = model(B, cut, k, False)[0]
        assert int(r.added) == sum(t.cnt.values()) and int(r.n_new) == len(t.cnt)
        t.check(what="lens of rfq_adapter_rows")
    finally:
        t.free(); gl.free(); dev.free()


# ---------------------------------------------------------------- test 5: hot values
def hot_cases():
    """(label, k, B, lens): 4096 rows of 150 x A at k = 25 (one value, count 516,096); random rows at k = 4 (at most 136 canonical values, every one hot); both
    mixed with random rows at k = 25, so that a workgroup's LDS table overflows into device memory"""
    rng = np.random.default_rng(77)
    polyA = [b"A" * 150] * 4096
    B, lens = S.rows_of(polyA, 160, "ascii", pad=ord("A"))
    yield "poly-A", 25, B, lens
    few = [S.rand_seq(rng, 150) for _ in range(64)]
    B, lens = S.rows_of([few[i % 64] for i in range(1024)], 160, "code", pad=0)
    yield "k 4", 4, B, lens
    rnd = [S.rand_seq(rng, 150) for _ in range(400)]
    mix = [(b"A" * 150, b"G" * 150, rnd[i % 400])[i % 3] if i % 7 else rnd[i % 400][:75] + b"A" * 75 for i in range(1536)]
    B, lens = S.rows_of(mix, 160, "ascii", pad=ord("C"))
    yield "a mix", 25, B, lens


def check_hot(codec, twice, paths=(None,)):
    """each case into fresh tables, on the GPU twice: the table is the model, and the two reads are identical - a condition the tree meets, not a rate.  (Counts past
    2^32 are not reached: a few-second test cannot add that often.)"""
    for label, k, B, lens in hot_cases():
        cnt, _, _ = model(B, lens, k, label == "k 4")
        if label == "poly-A":
            assert cnt == {0: 516096}
        if label == "k 4":
            assert len(cnt) <= 136 and min(cnt.values()) > 100
        if label == "a mix":
            assert len(cnt) > 2048 and max(cnt.values()) > 60000              # (more values than the LDS table has slots, and hot ones among them)
        for path in paths:
            reads = []
            for _ in range(2 if twice else 1):
                t = Table(codec, k, 2 * len(cnt))
                try:
                    t.add(B, lens, codes=label == "k 4", option=path, what="hot: %s" % label)
                    got = t.check(hist_len=4, what="hot: %s under %s" % (label, path or "default"))
                    reads.append((got["pairs"], got["hist"].tolist(), got["summary"]))
                finally:
                    t.free()
            assert all(r == reads[0] for r in reads), "two runs into fresh tables read differently"


# ---------------------------------------------------------------- test 6: formulations
def check_formulations(codec, labels=("17", "257", "1025")):
    """default, general, direct and collide give the same selected lists and histograms on the rows of the seams and of the hot values"""
    def rows():
        for label in labels:
            k, L, seqs, lens = seam_rows(label)
            B, _ = S.rows_of(seqs, L, "ascii")
            yield "seams %s" % label, k, B, lens, False
        for label, k, B, lens in hot_cases():                                 # (their first 600 rows: under collide ONE chain holds every value)
            yield label, k, B[:600], lens[:600], label == "k 4"
    for what, k, B, lens, codes in rows():
        reads = []
        cnt = model(B, lens, k, codes)[0]
        for form in FORMS:
            t = Table(codec, k, min(2 * len(cnt), 65536), "collide" if form == "collide" else None)
            try:
                t.add(B, lens, codes, option=form, what="%s under %s" % (what, form or "default"))
                got = t.check(hist_len=6, what="%s under %s" % (what, form or "default"))
                reads.append((got["pairs"], got["hist"].tolist(), got["summary"]))
                flags = int(np.frombuffer(t.g.body()[40:44], np.uint32)[0])
                assert flags == (1 if form == "collide" else 0), "the collide flag is recorded in the header"
            finally:
                t.free()
        assert all(r == reads[0] for r in reads), what


def check_option(codec, reset):
    from repaq_amd import RfqError
    assert OPTION in codec.option_names() and codec.get_option(OPTION) == ""
    for v in ("collide", "general", "direct"):
        codec.set_option(OPTION, v)
        assert codec.get_option(OPTION) == v
        reset(codec)
        assert codec.get_option(OPTION) == ""
    for bad in ("staged", "Direct", "1"):
        with R.pytest_raises(RfqError):
            codec.set_option(OPTION, bad)
    assert codec.get_option(OPTION) == ""
    # a table formatted under collide counts the same whatever the switch says later; more than 65536 slots are refused under it
    codec.set_option(OPTION, "collide")
    try:
        with R.pytest_raises(RfqError) as ei:
            codec.kmers_init(k=16, slots=65537, size_only=True)
        assert ei.value.code == E_ARG and "collide" in ei.value.message
    finally:
        codec.set_option(OPTION, None)


# ---------------------------------------------------------------- test 7: the read
def planted_counts(rng, k, counts):
    """rows of exactly k bases: value i (random, distinct, no two of them reverse complements) in counts[i] rows; returns (B, lens, Counter)"""
    seqs, seen = [], set()
    for c in counts:
        while True:
            s = S.rand_seq(rng, k); v = S.canon(S.digits(s, False))
            if v not in seen:
                seen.add(v); break
        seqs += [s if i % 2 else S.revcomp(s) for i in range(c)]
    B, lens = S.rows_of(seqs, k, "ascii")
    return B, lens, model(B, lens, k, False)[0]


def check_read(codec):
    from repaq_amd import RfqError
    rng = np.random.default_rng(78)
    k = 21
    counts = [1] * 5 + [2] * 4 + [3] * 3 + [7, 7, 8, 9, 40]
    B, lens, cnt = planted_counts(rng, k, counts)
    assert sorted(cnt.values()) == sorted(counts)
    t = Table(codec, k, 64)
    idx_bufs = []
    try:
        t.add(B, lens, what="planted counts")
        # min_count / max_count: c - 1, c, c + 1 around the planted counts; 0 and 1 are the same lower bound
        for c in (1, 2, 3, 7, 8, 40):
            for lo in (c - 1, c, c + 1):
                t.check(min_count=lo, hist_len=3, what="min_count %d" % lo)
                for hi in (c - 1, c, c + 1):
                    t.check(min_count=lo, max_count=hi, hist_len=0, what="min_count %d max_count %d" % (lo, hi))
        for hist_len in (1, 2, 7, 8, 9, 40, 41, 5000):                       # (one bin; the overflow bin at, in front of and behind planted counts; bins not in LDS)
            got = t.check(hist_len=hist_len, what="hist_len %d" % hist_len)
            assert int(got["hist"].sum()) == len(cnt)
        assert t.check(hist_len=1)["hist"][0] == len(cnt) and t.check(hist_len=2)["hist"].tolist() == [5, len(cnt) - 5]
        # size_only writes nothing
        g = W.Guarded(codec, 8 * len(cnt))
        try:
            q = codec.kmers_read(t.ptr, t.bytes, size_only=True, hist_len=4, d_hist=g.ptr, d_values=g.ptr, d_counts=g.ptr, list_cap=len(cnt), d_index=g.ptr, index_cap=1 << 20)
            assert int(q.n_selected) == len(cnt) and set(g.body()) == {0xA5}
        finally:
            g.free()
        # no room: nothing is written
        ns = len(selected(cnt, 2)); ib = 64 + 8 * 1024
        gv, gc, gh, gi = W.Guarded(codec, 8 * ns), W.Guarded(codec, 8 * ns), W.Guarded(codec, 8 * 4), W.Guarded(codec, ib)
        try:
            for list_cap, index_cap, need in ((ns - 1, ib, "need %d list entries" % ns), (ns, ib - 1, "%d index bytes" % ib), (0, 0, "need %d list entries" % ns)):
                with R.pytest_raises(RfqError) as ei:
                    codec.kmers_read(t.ptr, t.bytes, min_count=2, hist_len=4, d_hist=gh.ptr, d_values=gv.ptr, d_counts=gc.ptr, list_cap=list_cap, d_index=gi.ptr, index_cap=index_cap)
                assert ei.value.code == E_NOSPACE and need in ei.value.message, ei.value
                for x in (gv, gc, gh, gi):
                    assert x.guards_intact() and set(x.body()) <= {0xA5}, "a refused read wrote into an output"
            r = codec.kmers_read(t.ptr, t.bytes, min_count=2, hist_len=4, d_hist=gh.ptr, d_values=gv.ptr, d_counts=gc.ptr, list_cap=ns, d_index=gi.ptr, index_cap=ib)
            assert int(r.n_selected) == ns and all(x.guards_intact() for x in (gv, gc, gh, gi))
        finally:
            for x in (gv, gc, gh, gi):
                x.free()
        # the index: rfq_screen_rows on fresh rows gives the model's hits for set = the selected values; its n_kmers and S are those of rfq_screen_build on
        # references that spell out exactly those k-mers, one reference per k-mer
        fresh = [S.rand_seq(rng, 60) for _ in range(6)]
        for v, c in list(cnt.items())[::2]:
            d = np.base_repr(v, 4).rjust(k, "0").translate(str.maketrans("0123", "ACGT")).encode()
            assert S.canon(S.digits(d, False)) == v
            fresh.append(S.rand_seq(rng, 20) + (d if c % 2 else S.revcomp(d)) + S.rand_seq(rng, 19))
        Bf, lf = S.rows_of(fresh, 64, "ascii")
        for lo, hi in ((1, 0), (2, 0), (3, 8), (41, 0)):
            sel = selected(cnt, lo, hi)
            got = t.read(min_count=lo, max_count=hi, index=True); gi = got["index"]; idx_bufs.append(gi)
            refs = [np.base_repr(v, 4).rjust(k, "0").translate(str.maketrans("0123", "ACGT")).encode() for v, _ in sel]
            built = S.Index(codec, refs, k)
            try:
                hdr = np.frombuffer(gi.body()[:64], np.uint64); ref_hdr = np.frombuffer(built.g.body()[:64], np.uint64)
                assert hdr.tolist() == ref_hdr.tolist(), "the index's header is not what rfq_screen_build writes for these k-mers"
                assert int(hdr[3]) == len(sel) and int(hdr[2]) == pow2(2 * len(sel))
                e = S.expected(Bf, lf, {v for v, _ in sel}, k, False, min_hits=1)
                dev = S.dev_rows(codec, Bf, lf)
                try:
                    for path in S.PATHS:
                        codec.set_option(S.OPTION, path)
                        out, summ, _ = S.run(codec, dev, built, index=(gi.ptr, gi.n))
                        S.compare(out, summ, e, "the read's index, min %d max %d, %s:" % (lo, hi, path or "default"))
                    codec.set_option(S.OPTION, None)
                finally:
                    codec.set_option(S.OPTION, None)
                    dev.free()
                assert (e["summary"]["hits"] > 0) == bool(sel)
            finally:
                built.free()
        # an empty table reads as empty, its index is the empty set
        t.init()
        got = t.check(hist_len=3, what="an empty table")
        assert got["pairs"] == [] and got["hist"].tolist() == [0, 0, 0] and got["summary"]["index_slots"] == 1024
        got = t.read(index=True); gi = got["index"]; idx_bufs.append(gi)
        assert set(gi.body()[64:]) == {0} and int(np.frombuffer(gi.body()[:64], np.uint64)[3]) == 0
        dev = S.dev_rows(codec, Bf, lf)
        try:
            r = codec.screen_rows(*dev.adapter_args(), gi.ptr, gi.n)
            assert int(r.hits) == 0 and int(r.kmers) > 0
        finally:
            dev.free()
    finally:
        t.free()
        for g in idx_bufs:
            g.free()


# ---------------------------------------------------------------- test 8: a table that is full
def _good(codec):
    """what every refusal is followed by, on the same context: a table that counts as the model says"""
    rng = np.random.default_rng(9)
    B, lens = S.rows_of([S.rand_seq(rng, 50) for _ in range(5)], 50, "ascii")
    counted(codec, B, lens, 16, paths=(None,), what="after a refusal")


def check_full(codec):
    """S = 1024 and 3000 distinct k-mers: RFQ_E_NOSPACE with lost > 0, the call returns; the table is then RFQ_E_DATA for rows and for read; after rfq_kmers_init
    it counts again; the context's next unrelated call is right.  A bounded, refused call."""
    from repaq_amd import RfqError
    rng = np.random.default_rng(79)
    k = 25
    many = [S.rand_seq(rng, 124) for _ in range(30)]                          # 30 * 100 k-mers of random sequence: 3000 distinct values
    B, lens = S.rows_of(many, 128, "ascii")
    assert len(model(B, lens, k, False)[0]) == 3000
    few = S.rows_of(many[:3], 128, "ascii")
    for form in FORMS:
        t = Table(codec, k, 1024, "collide" if form == "collide" else None)
        dev = S.dev_rows(codec, B, lens); dev_few = S.dev_rows(codec, *few)
        try:
            codec.set_option(OPTION, form)
            with R.pytest_raises(RfqError) as ei:
                t.count(dev)
            m = re.search(r"(\d+) k-mers lost with (\d+) values in (\d+) slots", ei.value.message)
            assert ei.value.code == E_NOSPACE and m, ei.value
            lost, n_kmers, slots = (int(x) for x in m.groups())
            assert lost > 0 and lost + n_kmers == 3000 and slots == 1024 and n_kmers <= 1024, (form, lost, n_kmers)
            assert t.g.guards_intact()
            for call in (lambda: t.count(dev_few), lambda: t.read(), lambda: codec.kmers_read(t.ptr, t.bytes, size_only=True)):
                with R.pytest_raises(RfqError) as ei:
                    call()
                assert ei.value.code == E_DATA and "INCOMPLETE" in ei.value.message, ei.value
            codec.set_option(OPTION, None)
            t.init()
            t.add(*few, option=form, what="after rfq_kmers_init")
            t.check(what="a full table formatted again")
        finally:
            codec.set_option(OPTION, None)
            t.free(); dev.free(); dev_few.free()
    S._good(codec)                                                            # (the context's next unrelated calls: a screen build and a screen)


# ---------------------------------------------------------------- test 9: refusals
def check_init_refusals(codec):
    from repaq_amd import RfqError
    buf = W.Guarded(codec, 64 + 16 * 1024)
    need = 64 + 16 * 1024
    I = codec.kmers_init
    try:
        calls = ((E_ARG, "k must be", lambda: I(k=3, slots=10, d_table=buf.ptr, table_cap=need)),
                 (E_ARG, "k must be", lambda: I(k=32, slots=10, size_only=True)),
                 (E_ARG, "2^36", lambda: I(k=16, slots=(1 << 36) + 1, size_only=True)),
                 (E_ARG, "null d_table", lambda: I(k=16, slots=10)),
                 (E_ARG, "16-byte aligned", lambda: I(k=16, slots=10, d_table=C.c_void_p(buf.ptr.value + 8), table_cap=need)),
                 (E_NOSPACE, "need %d bytes" % need, lambda: I(k=16, slots=10, d_table=buf.ptr, table_cap=need - 1)),
                 (E_NOSPACE, "need %d bytes" % (64 + 16 * 2048), lambda: I(k=16, slots=1025, d_table=buf.ptr, table_cap=need)))
        for code, what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == code and what in ei.value.message, (what, ei.value)
            assert set(buf.body()) == {0xA5} and buf.guards_intact(), "a refused rfq_kmers_init wrote"
            _good(codec)
        assert int(I(k=16, slots=1 << 36, size_only=True).table_bytes) == 64 + 16 * (1 << 36)
        assert int(I(k=4, slots=0, size_only=True).slots) == 1024
    finally:
        buf.free()


def check_host_refusals(codec):
    from repaq_amd import RfqError
    rng = np.random.default_rng(81)
    t = Table(codec, 16, 2048)
    B, lens = S.rows_of([S.rand_seq(rng, 30) for _ in range(12)], 32, "ascii")
    n, L = B.shape
    dev = S.dev_rows(codec, B, lens, np.ones(n, np.uint8))
    buf = codec.dev_put(b"\0" * 16384); b = buf.value
    try:
        rows = dev.adapter_args(); tb = (t.ptr, t.bytes)

        def at(p, k):
            return C.c_void_p(p.value + k)
        D = codec.kmers_rows; Rd = codec.kmers_read
        calls = (("bad base_mode", lambda: D(*rows, *tb, base_mode=7)),
                 ("row_len must be >= 1", lambda: D(n, 0, dev.bases, dev.lens, *tb)),
                 ("null d_lens / d_bases", lambda: D(n, L, None, dev.lens, *tb)),
                 ("null d_lens / d_bases", lambda: D(n, L, dev.bases, None, *tb)),
                 ("d_table must be", lambda: D(*rows, None, t.bytes)),
                 ("d_table must be", lambda: D(*rows, at(t.ptr, 8), t.bytes - 8)),
                 ("d_table must be", lambda: D(*rows, t.ptr, 63)),
                 ("4-byte aligned", lambda: D(n, L, dev.bases, at(dev.lens, 2), *tb)),
                 ("4-byte aligned", lambda: D(*rows, *tb, d_kmers=C.c_void_p(b + 2))),
                 ("d_kmers overlaps the input rows->d_bases", lambda: D(*rows, *tb, d_kmers=at(dev.bases, n * L - 4))),
                 ("d_kmers overlaps the input d_in", lambda: D(*rows, *tb, d_in=dev.cand, d_kmers=dev.cand)),
                 ("d_kmers overlaps the input rows->d_lens", lambda: D(*rows, *tb, d_kmers=dev.lens)),
                 ("d_kmers overlaps the input d_table", lambda: D(*rows, *tb, d_kmers=at(t.ptr, t.bytes - 4))),
                 ("d_table overlaps the input rows->d_bases", lambda: D(n, L, at(t.ptr, 128), dev.lens, *tb)),
                 ("d_table overlaps the input d_in", lambda: D(*rows, *tb, d_in=at(t.ptr, 4096))),
                 ("too many rows", lambda: D(1 << 31, 1, dev.bases, dev.lens, *tb)),
                 ("d_table must be", lambda: Rd(None, t.bytes)),
                 ("d_table must be", lambda: Rd(at(t.ptr, 8), t.bytes - 8)),
                 ("d_table must be", lambda: Rd(t.ptr, 63)),
                 ("hist_len must be", lambda: Rd(*tb, hist_len=65537)),
                 ("hist_len must be", lambda: Rd(*tb, hist_len=0, d_hist=C.c_void_p(b))),
                 ("8-byte aligned", lambda: Rd(*tb, hist_len=4, d_hist=C.c_void_p(b + 4))),
                 ("8-byte aligned", lambda: Rd(*tb, d_values=C.c_void_p(b + 1), list_cap=4)),
                 ("8-byte aligned", lambda: Rd(*tb, d_counts=C.c_void_p(b + 2), list_cap=4)),
                 ("16-byte aligned", lambda: Rd(*tb, d_index=C.c_void_p(b + 8), index_cap=8256)),
                 ("d_hist overlaps the input d_table", lambda: Rd(*tb, hist_len=4, d_hist=at(t.ptr, t.bytes - 8))),
                 ("d_index overlaps the input d_table", lambda: Rd(*tb, d_index=at(t.ptr, 64), index_cap=8256)),
                 ("d_values overlaps the output d_counts", lambda: Rd(*tb, d_values=C.c_void_p(b), d_counts=C.c_void_p(b + 8), list_cap=4)),
                 ("d_hist overlaps the output d_index", lambda: Rd(*tb, hist_len=4, d_hist=C.c_void_p(b + 64), d_index=C.c_void_p(b), index_cap=8256)))
        for what, f in calls:
            with R.pytest_raises(RfqError) as ei:
                f()
            assert ei.value.code == E_ARG and what in ei.value.message, (what, ei.value)
            _good(codec)
        assert t.g.guards_intact() and set(t.g.body()[64:]) == {0}, "a refused call wrote into the table"
        # (no rows at all are no error and take no row pointers; the table's counts come back)
        t.add(B, lens, what="after the refusals")
        r = D(0, 0, None, None, *tb)
        assert summary_of(r, ROWS_FIELDS) == dict(dict.fromkeys(ROWS_FIELDS, 0), n_kmers=len(t.cnt), total=sum(t.cnt.values()))
        t.check(what="after the refusals")
    finally:
        dev.free(); codec.dev_free(buf); t.free()


def check_bad_table(codec):
    """RFQ_E_DATA for a header rfq_kmers_init does not write - a zeroed one, a screen index, every field off -; a table whose slots the test has filled with
    non-empty garbage: the call returns (refused: every k-mer is lost), walks are bounded, nothing outside the buffer is touched"""
    from repaq_amd import RfqError
    rng = np.random.default_rng(82)
    k = 16
    ref = S.rand_seq(rng, 100)
    B, lens = S.rows_of([ref[:60], S.rand_seq(rng, 60), ref[40:]], 64, "ascii")
    dev = S.dev_rows(codec, B, lens)
    t = Table(codec, k, 1024)
    idx = S.Index(codec, [ref], k)
    copies = []
    try:
        t.add(B, lens, what="the good table")
        img = bytes(t.g.body())
        hdr = np.frombuffer(img[:64], np.uint32).copy()                       # magic (2 words), version, k, S (2), n_kmers (2), total (2), flags
        assert hdr[3] == k and hdr[4] == 1024 and hdr[6] == len(t.cnt) and hdr[8] == sum(t.cnt.values()) and hdr[10] == 0

        def variant(body=None, **words):
            h = hdr.copy()
            for w, v in words.items():
                h[int(w[1:])] = v
            g = W.Guarded(codec, len(img)); copies.append(g)
            codec._check(codec._L.rfq_copy_h2d(codec._h, g.ptr, h.tobytes() + (img[64:] if body is None else body), len(img)))
            return g
        for what, words in (("does not begin with the header", dict(w0=int(hdr[0]) ^ 1)), ("does not begin with the header", dict(w2=2)), ("the table's k", dict(w3=0)),
                            ("the table's k", dict(w3=32)), ("slot count", dict(w4=1000)), ("slot count", dict(w4=0)), ("slot count", dict(w4=2048)),
                            ("slot count", dict(w5=1)), ("INCOMPLETE", dict(w10=2)),
                            ("does not begin with the header", dict(w0=0, w1=0, w2=0, w3=0, w4=0, w5=0, w6=0, w7=0, w8=0, w9=0, w10=0))):
            g = variant(**words)
            for call in (lambda: t.count(dev, table=(g.ptr, g.n)), lambda: t.read(table=(g.ptr, g.n))):
                with R.pytest_raises(RfqError) as ei:
                    call()
                assert ei.value.code == E_DATA and what in ei.value.message, (what, words, ei.value)
            assert g.guards_intact() and g.body()[64:] == img[64:]
            _good(codec)
        # a screen index handed in as a table; a table handed to rfq_screen_rows
        for call in (lambda: t.count(dev, table=(idx.ptr, idx.bytes)), lambda: t.read(table=(idx.ptr, idx.bytes))):
            with R.pytest_raises(RfqError) as ei:
                call()
            assert ei.value.code == E_DATA and "does not begin with the header" in ei.value.message, ei.value
        with R.pytest_raises(RfqError) as ei:
            S.run(codec, dev, idx, index=(t.ptr, t.bytes))
        assert ei.value.code == E_DATA
        # a copy of the good table is as good as the table
        g = variant()
        assert t.read(table=(g.ptr, g.n), hist_len=4)["pairs"] == selected(t.cnt)
        # slots that do not hold what the header counts
        g = variant(w6=int(hdr[6]) + 1)
        with R.pytest_raises(RfqError) as ei:
            t.read(table=(g.ptr, g.n))
        assert ei.value.code == E_DATA and "written over" in ei.value.message
        # every slot taken by garbage, none of it a k-mer of these rows (the values are above 4^16), and counts of garbage: every walk ends after min(S, W) steps
        full = ((np.arange(1024, dtype=np.uint64) + np.uint64(1 << 40)) | np.uint64(1 << 63)).tobytes() + rng.integers(1, 1 << 62, 1024, dtype=np.uint64).tobytes()
        for path in PATHS:
            g = variant(body=full)
            codec.set_option(OPTION, path)
            with R.pytest_raises(RfqError) as ei:
                t.count(dev, table=(g.ptr, g.n))
            codec.set_option(OPTION, None)
            assert ei.value.code == E_NOSPACE and " k-mers lost" in ei.value.message, ei.value
            assert g.guards_intact() and g.body()[64:] == full, "a walk over garbage wrote into the slots or the counts"
            with R.pytest_raises(RfqError) as ei:
                t.read(table=(g.ptr, g.n))
            assert ei.value.code == E_DATA
            _good(codec)
        # garbage without bit 63 and counts of 0, under a header that was not marked: the read returns, inside its buffers
        junk = rng.integers(1, 1 << 62, 1024, dtype=np.uint64).tobytes() + bytes(8 * 1024)
        g = variant(body=junk, w6=0, w7=0, w8=0, w9=0)
        got = t.read(table=(g.ptr, g.n), hist_len=4)
        assert got["pairs"] == [] and got["summary"]["n_kmers"] == 0 and g.guards_intact()
    finally:
        codec.set_option(OPTION, None)
        dev.free(); t.free(); idx.free()
        for g in copies:
            g.free()


DEVICE_REFUSALS = [(v, row) for v in ("negative", "row_len_plus_1") for row in ("first", "last", "middle")]
DEVICE_REFUSAL_IDS = ["%s_%s" % x for x in DEVICE_REFUSALS]


def check_device_refusal(codec, label):
    from repaq_amd import RfqError
    value, where = DEVICE_REFUSALS[DEVICE_REFUSAL_IDS.index(label)]
    rng = np.random.default_rng(83)
    t = Table(codec, 15, 1 << 15)
    try:
        for L, n in ((24, 300), (300, 10), (1100, 6)):
            B = np.frombuffer(S.rand_seq(rng, n * L), np.uint8).reshape(n, L); lens = rng.integers(0, L + 1, n).astype(np.int32)
            row = dict(first=0, last=n - 1, middle=n // 2)[where]
            lens[row] = -1 if value == "negative" else L + 1
            for cand in (None, (np.arange(n) != row).astype(np.uint8)):      # (every row is judged, counted or not)
                dev = S.dev_rows(codec, B, lens, cand, shift=1)
                try:
                    for path in PATHS:
                        codec.set_option(OPTION, path)
                        for want_kmers in (False, True):
                            with R.pytest_raises(RfqError) as ei:
                                t.count(dev, want_kmers=want_kmers)
                            assert ei.value.code == E_ARG and "first such row: %d)" % row in ei.value.message, (label, L, ei.value)
                        codec.set_option(OPTION, None)
                    # the table holds the other counted rows' k-mers and its header says so: the read takes it
                    q = codec.kmers_read(t.ptr, t.bytes, size_only=True)
                    assert int(q.total) > 0
                    _good(codec)
                finally:
                    codec.set_option(OPTION, None)
                    dev.free()
        lens = np.full(n, L, np.int32); lens[1] = -5; lens[4] = L + 1
        dev = S.dev_rows(codec, B, lens)
        try:
            with R.pytest_raises(RfqError) as ei:
                t.count(dev)
            assert "first such row: 1)" in ei.value.message
        finally:
            dev.free()
    finally:
        t.free()


# ---------------------------------------------------------------- test 10: state and composition
def check_state(codec):
    """a count (init, rows, read) between two rfq_dedup_rows calls and two rfq_rows_to_text calls on one context leaves their results byte-identical"""
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
        rng = np.random.default_rng(85)
        Bs, ls = S.rows_of([S.rand_seq(rng, 300) for _ in range(9)], 300, "ascii")
        counted(codec, Bs, ls, 21, what="between the calls")
        assert calls() == first, "a count between them changed what rfq_dedup_rows or rfq_rows_to_text give"
    finally:
        dd.free(); dt.free()
    t = Table(codec, 21, 8192)
    try:
        assert [nm for nm, _ in codec.timings()] == ["kmers:init"]
        t.add(Bs, ls)
        t.read()
        assert [nm for nm, _ in codec.timings()] == ["kmers:read"]
    finally:
        t.free()


COMPOSE_K = 21


def compose_texts(pairs=90, seed=15):
    """two small texts (R1, R2) of fragments with adapters behind them: a third of the fragments come from a 300-base repeat (their k-mers are seen again and
    again), the others are random - every one of their k-mers is seen in this pair alone -, a few reads end in low scores"""
    import _adapter as A
    rng = np.random.default_rng(seed)
    repeat = S.rand_seq(rng, 300)
    a = (A.AD1 + b"ACGTTGCATTGACCA" * 12, A.AD2 + b"TTGACGGATCAGGCA" * 12)
    out = [[], []]
    for i in range(pairs):
        ins = int(rng.integers(60, 260))
        if i % 3 == 0:
            j = int(rng.integers(0, 300 - min(ins, 200))); f = repeat[j:j + min(ins, 200)]
            f = S.revcomp(f) if i % 2 else f
        else:
            f = S.rand_seq(rng, ins)
        for m, fr in ((0, f), (1, S.revcomp(f))):
            s = (fr + a[m])[:150]
            q = np.clip(38 - np.arange(150) * int(rng.integers(0, 30)) // 150 + rng.integers(-4, 5, 150), 2, 41).astype(np.uint8)
            out[m].append(b"@frag.%d %d/%d\n" % (i + 1, i, m + 1) + s + b"\n+\n" + bytes(q + 33) + b"\n")
    return out


def compose_expected(t1, t2, ca, cj):
    """the chain on the host: adapter removal, the judge on the shortened reads, a Counter over the judge's rows (each row on its own), the values seen at least
    twice, the pairs of the judge whose k-mers are at least half among them, their texts in the judge's windows; returns (text 1, text 2, pairs kept, Counter,
    kmers [n], cut lengths, the judge's keep)"""
    import _adapter as A
    import _judge as J
    rows = [rec.split(b"\n")[:4] for pair in zip(t1, t2) for rec in pair]
    L = max(len(r[1]) for r in rows); n = len(rows)
    B = np.zeros((n, L), np.uint8); lens = np.array([len(r[1]) for r in rows], np.int32)
    for i, r in enumerate(rows):
        B[i, :len(r[1])] = np.frombuffer(r[1], np.uint8)
    cut = A.expected(B, lens, ca, False)["length"]
    keep = np.zeros(n, np.uint8); win = []
    for g in range(n):
        name, s, _, q = rows[g]
        kk, a, m, _, _ = J.judge_row(list(s), [x - 33 for x in q], int(cut[g]), cj, False)
        keep[g] = 1 if kk else 0; win.append((a, m))
    cnt, kmers, _ = model(B, cut, COMPOSE_K, False, keep)
    sel = {v for v, c in cnt.items() if c >= 2}
    out = [[], []]
    for i in range(0, n, 2):
        if not (keep[i] and keep[i + 1] and win[i][1] >= cj["min_len"] and win[i + 1][1] >= cj["min_len"]):
            continue
        vs = [v for g in (i, i + 1) for v in S.kmers_of(S.digits(rows[g][1][:int(cut[g])], False), COMPOSE_K)]
        H = sum(v in sel for v in vs)
        if not (H >= 1 and 100 * H >= 50 * len(vs)):
            continue
        for m in (0, 1):
            name, s, _, q = rows[i + m]; a, l = win[i + m]
            out[m].append(name + b"\n" + s[a:a + l] + b"\n+\n" + q[a:a + l] + b"\n")
    return b"".join(out[0]), b"".join(out[1]), len(out[0]), cnt, kmers, cut, keep
