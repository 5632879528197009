"""Shared helpers of the history tests (tests/test_emu_history.py on the SIMT interpreter, tests/test_gpu_history.py on the MI355X): what a context carries
from one call to the next (rfq_ctx: rec_per_byte / lazy_block, mixed_lengths, dense_ok, e3_pieces_failed, mirror_block, the qplane_* bookkeeping, 120 buffers that
only grow, the context-owned results of the rows family) is pinned by running every input behind every other one on ONE context.

The order is an Eulerian circuit of the complete digraph with loops (euler): k * k + 1 calls see each of the k * k ordered pairs (predecessor, input) once.  The
expected results never come from the library: _oracle.encode_file gives the image, _oracle.decode_file of that image the text, both computed once (inputs())."""
import collections
import threading

import numpy as np

import _engine as E
import _oracle as O
import _sections


def euler(k):
    """k * k + 1 indices in which every ordered pair (a, b) of range(k), a == b included, is adjacent exactly once (Hierholzer on the complete digraph with loops)"""
    left = {a: list(range(k)) for a in range(k)}                             # the edges a -> b not walked yet
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == k * k + 1 and out[0] == out[-1], (k, len(out))
    assert len(set(zip(out, out[1:]))) == k * k, k
    return out


# ---------------------------------------------------------------- the inputs
# want: the oracle's image; text: the oracle's decode of it (a pair of texts where `split`); caller: the decode goes into caller buffers (the emitter is launched ahead
# of the host's look at the status); state: the context state the input is there for; enc_mark / dec_mark: stage names of codec.timings() a FRESH context must (with
# "!": must not) show on its first encode / decode of it; enc2_mark: the same for a second encode on that context (`lazy_index`: the index without a read-back, which the
# context can do once it knows the records per byte and which a text that has to be normalised or ends at an empty line never gets).  What no stage name shows is
# asserted on the oracle's image instead (add(check=...)): the chunk flags, the header's table.
Input = collections.namedtuple("Input", "name fq1 fq2 paired cb want text split caller state enc_mark dec_mark enc2_mark")
_INPUTS = None


def _text(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def _records(fq):
    ln = fq.split(b"\n")
    assert ln[-1] == b""
    return [ln[i:i + 4] for i in range(0, len(ln) - 1, 4)]


def _qual_recs(n, quals, seed):
    """n SE150 records whose quality bytes are drawn evenly from `quals` (the text of _engine.check_every_repeat_in_one_call)"""
    import random
    rng = random.Random(seed)

    def rec(i):
        seq = bytes(rng.choice(b"ACGT") for _ in range(150)); q = bytes(rng.choice(quals) for _ in range(150))
        return b"@M:1:FC:1:%d:%d:%d 1:N:0:AC\n" % (1101 + i // 500, rng.randrange(1000, 30000), rng.randrange(1000, 60000)) + seq + b"\n+\n" + q + b"\n"
    return b"".join(rec(i) for i in range(n))


def _rare_recs(n, seed):
    """n SE150 records: quality 'F' but for about 1 byte in 400, drawn from ':', ',' and '5'; from record 200 on (chunk 0 ends before it at 20,000 bases a chunk)
    one byte in 1500 is '<', which the header's table - made from chunk 0 - does not hold: an exception"""
    import random
    rng = random.Random(seed); out = []
    for i in range(n):
        seq = bytes(rng.choice(b"ACGT") for _ in range(150)); q = bytearray(b"F" * 150)
        for j in range(150):
            if rng.random() < 1 / 400:
                q[j] = rng.choice(b":,5")
            if i >= 200 and rng.random() < 1 / 1500:
                q[j] = ord("<")
        out.append(b"@M:1:FC:1:%d:%d:%d 1:N:0:AC\n" % (1101 + i // 500, rng.randrange(1000, 30000), rng.randrange(1000, 60000)) + seq + b"\n+\n" + bytes(q) + b"\n")
    return b"".join(out)


def _rare_planes_are_reached(fq1, want):
    """Match-mask mode takes files of up to four coded values and keeps at most THREE dense planes (rfq_encode.hip: M.nd = min(n_normal, 3), two where the tile has no
    room for three - reads of 150 bases); the other coded values and every byte outside the header's table (the exception plane) are set bit by bit in RARE planes,
    listed in rare[] and zeroed again by k_rare_cleanup.  This text has four coded values - three that occur in every chunk and the 0xFF entry the reference appends
    for a file without N bases - and, in every chunk behind the first, bytes outside the table: bits in the exception plane whatever the dense planes are, and in a
    coded value's plane where there are two.  Few enough per chunk that rare[] stays a list (<= G2_RARE_LIST = 255 words): the cleanup's sparse branch - its other
    branch, the whole extent, is four_quals' (a quarter of all bytes in the fourth plane)."""
    h, chunks = _sections.parse(want)
    assert sorted(h.normal) == sorted(b":,5\xff") and len(chunks) >= 3, (h.normal, len(chunks))
    quals = [r[3] for r in _records(fq1)]; at = 0
    for k, c in enumerate(chunks):
        q = b"".join(quals[at:at + c.reads]); at += c.reads
        counts = [q.count(bytes([v])) for v in b":,5"]; exc = q.count(b"<")
        assert min(counts) >= 1 and (exc >= 1) == (k > 0) and sum(counts) + exc <= 255, (k, counts, exc)
    assert at == len(quals)


def _chunk_flags(test):
    """a check for add(): `test(flags, reads)` holds for every chunk of the oracle's image"""
    def check(fq1, want):
        _, chunks = _sections.parse(want)
        assert chunks and all(test(c.flags, c.reads) for c in chunks), [(hex(c.flags), c.reads) for c in chunks]
    return check


def inputs():
    """the dozen texts, made once and never changed"""
    global _INPUTS
    if _INPUTS is not None:
        return _INPUTS
    made = []

    def add(name, fq1, fq2, paired, cb, state, enc_mark=(), dec_mark=(), enc2_mark=(), caller=False, lossless=True, check=None):
        want = O.encode_file(fq1, fq2, paired, cb)
        if check:
            check(fq1, want)
        split = paired == O.PE_TWO_FILES
        text = O.decode_file(want, split)
        if lossless:
            assert text == ((fq1, fq2) if split else fq1), name
        size, chunks = len(fq1) + len(fq2), len(O.chunk_table(want)) - 1
        if name != "three_records":
            assert 100_000 <= size <= 350_000 and 2 <= chunks <= 6 and 10_000 <= cb <= 30_000, (name, size, chunks, cb)
        made.append(Input(name, fq1, fq2, paired, cb, want, text, split, caller, state, tuple(enc_mark), tuple(dec_mark), tuple(enc2_mark)))

    a, b = O.gen(O.NOVA_PE150, 400, seed=11)
    add("pe150", a, b, O.PE_TWO_FILES, 30000, "mirrored index", enc_mark=("mirror_index", "!mirror_fallback"), enc2_mark=("mirror_index", "lazy_index"))
    # (tests/test_mirror_index.py::test_names_of_other_lengths_fall_back: one name of R2 a byte longer, the next a byte shorter - sizes equal, two line ends moved)
    a, b = O.gen(O.NOVA_PE150, 330, seed=19)
    r2 = _records(b); r2[170][0] += b"A"; r2[171][0] = r2[171][0][:-1]; b = _text(r2)
    assert len(a) == len(b)
    add("pe_unmirrored", a, b, O.PE_TWO_FILES, 30000, "mirror_block", enc_mark=("mirror_fallback", "!mirror_index"))
    a, _ = O.gen(O.SE_VAR, 500, seed=13)
    add("se_var", a, b"", O.SE, 15000, "mixed_lengths", check=_chunk_flags(lambda fl, n: not fl & _sections.C_READ_LEN_SAME))
    a, b = O.gen(O.BGI_PE100, 450, seed=14, n_quals=40)
    add("bgi_q40", a, b, O.PE_TWO_FILES, 20000, "no match masks (dense_ok stays down)", enc_mark=("!quality_masks",))
    add("four_quals", _qual_recs(900, b"F:,5", 5), b"", O.SE, 30000, "arenas sized too small: the room repeat", enc_mark=("retry_room", "quality_masks"))
    a = _rare_recs(600, 6)
    add("rare_quals", a, b"", O.SE, 20000, "rare planes: exceptions and a coded value beyond the dense ones, a short rare[] list per chunk (k_rare_cleanup)",
        enc_mark=("quality_masks",), check=_rare_planes_are_reached)
    # (the `mixed` text of _engine.check_pieces_remembered_behind_speculative_emit, with 60 long names for its 80: that test has ONE chunk of 900 reads, here a chunk
    # is 300 reads, and plan_fused sizes the name tile by the chunk's AVERAGE name - 80 names of 114 bytes among 300 average 41 bytes, which selects the 13 KB tile
    # that holds 64 of them: no retry, no state.  60 average 35 bytes: the 3 KB tile, which a run of 27 long names overflows)
    a = E.handmade(900, lambda i: ("SRR0123456.%d" % i) if not 400 <= i < 460 else ("L" * 110 + "%d" % i), lambda i: 100, lambda i: "+", seed=4,
                   qual_of=lambda i, j: "F" if (i + j) % 29 else ",")
    add("long_names", a, b"", O.SE, 30000, "e3_pieces_failed", dec_mark=("emit", "emit_expanded"), caller=True)
    a, _ = O.gen(O.SE_VAR, 400, seed=17)
    add("crlf", a.replace(b"\n", b"\r\n"), b"", O.SE, 15000, "the normalising path", lossless=False, enc2_mark=("!lazy_index",))
    a = _qual_recs(500, b"FFFFFF:,", 7)
    add("empty_line", a + b"\n" + _qual_recs(3, b"FFFFFF:,", 8), b"", O.SE, 20000, "the repeat that ends the input at an empty line", lossless=False, enc2_mark=("!lazy_index",))
    a, _ = O.gen(O.NOVA_PE150, 250, seed=18, interleaved=True)
    add("interleaved", a, b"", O.PE_INTERLEAVED, 20000, "pairs in one text", enc2_mark=("lazy_index",), check=_chunk_flags(lambda fl, n: fl & _sections.C_PE_INTERLEAVED))
    a, _ = O.gen(O.NOVA_SE150, 970, seed=15)
    add("se150_big", a, b"", O.SE, 30000, "the buffers grow (rec_per_byte of a uniform file)", enc2_mark=("lazy_index",),
        check=_chunk_flags(lambda fl, n: fl & _sections.C_READ_LEN_SAME))
    a, _ = O.gen(O.NOVA_SE150, 3, seed=16)
    add("three_records", a, b"", O.SE, 30000, "buffers far larger than the batch", enc2_mark=("lazy_index",), check=_chunk_flags(lambda fl, n: n == 3))
    assert max(len(i.fq1) + len(i.fq2) for i in made) == len(made[10].fq1) and made[10].name == "se150_big"
    _INPUTS = made
    return made


def by_name(name):
    return next(i for i in inputs() if i.name == name)


def marks_ok(marks, rules):
    return all((r[1:] not in marks) if r.startswith("!") else (r in marks) for r in rules)


# ---------------------------------------------------------------- where two images differ
def where(want: bytes, off: int):
    """(chunk, section) of the oracle's image `want` that byte `off` lies in"""
    try:
        h, chunks = _sections.parse(want)
    except Exception as e:                                                   # (the message must not get lost in a second failure)
        return "?", "unparsed (%s)" % e
    if off < h.len:
        return "-", "header"
    for k, c in enumerate(chunks):
        if c.off <= off < c.off + c.total:
            r = off - c.off
            ends = (("sizes", c.fixed), ("length arrays", c.len_arrays_end), ("lane/tile/x/y", c.coords_end), ("names/strand", c.qual_off - c.seq_size),
                    ("sequence", c.qual_off), ("quality", c.qual_off + c.qual_size), ("overlap/N positions", c.total))
            return k, next(name for name, end in ends if r < end)
    return "?", "behind the last chunk"


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    x = np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n)
    return int(np.argmax(x))


def image_diff(got: bytes, want: bytes):
    """'' when equal; otherwise the first differing offset and the chunk and section of the oracle's image it lies in"""
    if got == want:
        return ""
    off = first_diff(got, want)
    chunk, section = where(want, off)
    return "%d bytes for %d, first difference at offset %d: chunk %s, section %s" % (len(got), len(want), off, chunk, section)


def text_diff(got: bytes, want: bytes):
    if got == want:
        return ""
    off = first_diff(got, want)
    return "%d bytes for %d, first difference at offset %d (record %d)" % (len(got), len(want), off, want[:off].count(b"\n") // 4)


# ---------------------------------------------------------------- one step of a circuit
def encode_step(codec, inp):
    """'' or what is wrong with the context's image of the input"""
    got = E.encode(codec, inp.fq1, inp.fq2, inp.paired, inp.cb)
    return image_diff(got, inp.want)


def decode_step(codec, inp):
    """'' or what is wrong with the context's text(s) of the oracle's image"""
    caps = None
    if inp.caller:
        caps = (len(inp.text[0]) + 64, len(inp.text[1]) + 64) if inp.split else (len(inp.text) + 64, 0)
    got = codec.decode_bytes(inp.want, split_pe=inp.split, out_caps=caps)
    if inp.split:
        return text_diff(got[0], inp.text[0]) or text_diff(got[1], inp.text[1])
    return text_diff(got, inp.text)


def check_markers(make_codec, inp):
    """the input reaches the state it is there for: on a fresh context the first encode / decode (and the second encode) shows its stage markers, and every result is the oracle's"""
    c = make_codec()
    try:
        bad = encode_step(c, inp)
        marks = {n for n, _ in c.timings()}
        assert not bad, (inp.name, bad)
        assert marks_ok(marks, inp.enc_mark), (inp.name, inp.enc_mark, sorted(marks))
        if inp.enc2_mark:
            bad = encode_step(c, inp)
            marks = {n for n, _ in c.timings()}
            assert not bad, (inp.name, "second encode", bad)
            assert marks_ok(marks, inp.enc2_mark), (inp.name, "second encode", inp.enc2_mark, sorted(marks))
    finally:
        c.close()
    c = make_codec()
    try:
        bad = decode_step(c, inp)
        marks = {n for n, _ in c.timings()}
        assert not bad, (inp.name, bad)
        assert marks_ok(marks, inp.dec_mark), (inp.name, inp.dec_mark, sorted(marks))
    finally:
        c.close()


def walk(codec, seq, kind_of, start=0, stop=None, state=None):
    """steps start .. stop of the sequence on `codec`; kind_of(i) -> "enc" / "dec".  Every failing step is collected (the context goes on: what a wrong state does to
    the calls behind it is part of the picture) and the assert names the input, the call in front of it and - encode state is left by the last ENCODE, decode state
    by the last decode - the last call of its own kind, with the place.  state: what walk returned for the steps in front of `start` on this context."""
    ins = inputs(); bad = []
    state = dict(state or {})
    stop = len(seq) if stop is None else stop
    for i in range(start, stop):
        inp = ins[seq[i]]; kind = kind_of(i)
        msg = (encode_step if kind == "enc" else decode_step)(codec, inp)
        if msg:
            marks = sorted(n for n, _ in codec.timings())
            prev, same = state.get("prev"), state.get(kind)
            behind = (prev or "a fresh context") + ("" if same == prev else ", the last %s being %s" % (kind, same or "none"))
            bad.append("step %d: %s of %s behind %s: %s; stages %s" % (i, kind, inp.name, behind, msg, marks))
        state["prev"] = state[kind] = "%s of %s" % (kind, inp.name)
    assert not bad, "%d of %d steps differ from the oracle:\n%s" % (len(bad), stop - start, "\n".join(bad[:12]))
    return state


KINDS = {"encode": lambda i: "enc", "decode": lambda i: "dec", "mixed": lambda i: "enc" if i % 2 else "dec"}


# ---------------------------------------------------------------- one file in two batches
def check_two_batches(codec, inp, other):
    """`inp` (one text) split at a record boundary: the first half with final=False, flush_all=True, a decode of `other`'s image on the same context, the second half
    with emit_header=False - the concatenation is the oracle's image of the whole text.  The boundary is the record at which the oracle's image ends a chunk (the one
    nearest the middle): flush_all ends a chunk where the batch ends, so at any other record the two batches make a valid image of the text, but not the oracle's."""
    from repaq_amd import nolb_threshold
    assert inp.paired == O.SE and b"\r" not in inp.fq1
    _, chunks = _sections.parse(inp.want)
    assert len(chunks) >= 2
    recs = _records(inp.fq1); cut = len(_text(recs[:sum(c.reads for c in chunks[:len(chunks) // 2])]))
    assert 0 < cut < len(inp.fq1)
    th = nolb_threshold(len(inp.fq1), inp.fq1.endswith(b"\n"))
    codec.clearHeader()
    d = codec.dev_put(inp.fq1[:cut])
    try:
        r = codec.encode(d, cut, None, 0, O.SE, inp.cb, final=False, flush_all=True, nolb_from1=th)
        assert r.consumed1 == cut, (r.consumed1, cut)
        first = codec.dev_get(r.d_rfq, r.rfq_len)
    finally:
        codec.dev_free(d)
    hdr = codec.header()
    msg = decode_step(codec, other)
    assert not msg, (other.name, msg)
    # (a decode with has_header parses the image's header and SETS it - include/rfq_hip.h, rfq_decode_args - so the file in progress takes its own back, the way a
    # worker of the host queue takes the first range's: rfq_get_header -> rfq_set_header.  What the context knew about the file is gone with it: new_file())
    assert codec.header() != hdr
    codec.setHeader(hdr)
    d = codec.dev_put(inp.fq1[cut:])
    try:
        r = codec.encode(d, len(inp.fq1) - cut, None, 0, O.SE, inp.cb, emit_header=False, file_off1=cut, nolb_from1=th)
        second = codec.dev_get(r.d_rfq, r.rfq_len)
    finally:
        codec.dev_free(d)
    return first + second


# ---------------------------------------------------------------- threads
def run_threads(jobs, timeout_s=120.0):
    """every job (a callable) on a host thread of its own, released together; an exception of any thread is raised here, a thread that does not come back fails"""
    barrier = threading.Barrier(len(jobs)); errors = [None] * len(jobs)

    def body(i):
        try:
            barrier.wait(timeout_s)
            jobs[i]()
        except BaseException as e:                                           # noqa: BLE001 (handed to the main thread)
            errors[i] = e
    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout_s)
    hung = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not hung, "threads %s did not come back within %.0f s" % (hung, timeout_s)
    for i, e in enumerate(errors):
        if e is not None:
            raise AssertionError("thread %d: %s: %s" % (i, type(e).__name__, e)) from e


# ---------------------------------------------------------------- the calls circuit: every KIND of call behind every other one
# One fixed small input per kind.  Every call goes through the helper its own tests use, which compares it with a host loop or the oracle EVERY time; what it returns
# (every output's bytes) must also equal what the same call gave first.  Context-owned results (rfq_decode_names' names_blob / names_off, rfq_rows_to_text's rows_txt,
# the encoder's and decoder's own result buffers): include/rfq_hip.h says "result pointers stay valid until the next call on the same context" - the next call
# invalidates them, so each is read BEFORE the next kind's call is issued, inside its own step.
CALL_KINDS = ("encode", "decode", "scan", "first_diff", "decode_rows", "decode_names", "text_rows", "select_rows", "judge_rows", "adapter_rows", "merge_rows",
              "rows_to_text", "encode_rows")


class Calls:
    """the fixtures of the calls circuit and their host references, made once"""
    def __init__(self):
        import _adapter as A
        import _judge as J
        import _merge as M
        import _names as N
        import _rows as W
        import _rows_enc as R
        import _select as S
        import _text_rows as T
        self.mod = dict(A=A, J=J, M=M, N=N, W=W, R=R, S=S, T=T)
        self.fq1, self.fq2 = O.gen(O.NOVA_PE150, 70, seed=21)
        self.paired, self.cb = O.PE_TWO_FILES, 10000
        self.want = O.encode_file(self.fq1, self.fq2, self.paired, self.cb)
        assert O.decode_file(self.want, True) == (self.fq1, self.fq2) and len(O.chunk_table(self.want)) - 1 >= 3
        # scan: a chunk ends where its last record ends in each file (the oracle's image says how many reads each chunk holds: both mates' together)
        _, chunks = _sections.parse(self.want)
        nl1 = [i + 1 for i, c in enumerate(self.fq1) if c == 10]; nl2 = [i + 1 for i, c in enumerate(self.fq2) if c == 10]
        pairs = np.cumsum([c.reads // 2 for c in chunks])
        self.scan_want = (len(chunks), [nl1[4 * int(p) - 1] for p in pairs], [nl2[4 * int(p) - 1] for p in pairs])
        # first_diff: two texts that differ in one byte behind the first 64 KiB
        self.cmp_a = self.fq1 * 4; self.cmp_at = 70_001
        b = bytearray(self.cmp_a); b[self.cmp_at] ^= 1; self.cmp_b = bytes(b)
        self.rows_want = W.expected(self.want)
        self.names_want = N.expected(self.want)
        self.recs = T.expect(self.fq1, self.fq2, self.paired, self.cb)[1]
        self.rows = R.rows_of(self.fq1, self.fq2, self.paired, extra="x16")
        B, Q, lens, names = self.rows; n = len(lens); rng = np.random.default_rng(31)
        self.sel = dict(keep=(rng.random(n) < 0.8).astype(np.uint8), start=rng.integers(0, 20, n).astype(np.int32), length=rng.integers(0, 120, n).astype(np.int32),
                        pairs=True, min_len=30)
        self.j_rows = J.random_rows(257, 150, 41, codes=False); self.j_crit = dict(J.STEPS)["all"]
        self.j_want = J.expected(*self.j_rows, self.j_crit, False)
        self.a_rows = A.random_pairs(33, 150, 43, codes=True); self.a_crit = A.shape_criteria(150)[2][1]
        self.a_want = A.expected(*self.a_rows, self.a_crit, True)
        self.m_rows = M.random_pairs(40, 64, 47, codes=False)
        self.m_want = M.expected(*self.m_rows, False)

    # each returns every output's bytes, as something that compares with ==
    def encode(self, c):
        got = E.encode(c, self.fq1, self.fq2, self.paired, self.cb)
        assert got == self.want, image_diff(got, self.want)
        return got

    def decode(self, c):
        got = c.decode_bytes(self.want, split_pe=True)
        assert got == (self.fq1, self.fq2), text_diff(got[0], self.fq1) or text_diff(got[1], self.fq2)
        return got

    def scan(self, c):
        d1 = c.dev_put(self.fq1); d2 = c.dev_put(self.fq2)
        try:
            r, e1, e2 = c.scan(d1, len(self.fq1), d2, len(self.fq2), self.paired, self.cb, final=True)
        finally:
            c.dev_free(d1); c.dev_free(d2)
        got = (r.n_chunks, e1, e2)
        assert got == self.scan_want, (got, self.scan_want)
        return got

    def first_diff(self, c):
        da = c.dev_put(self.cmp_a); db = c.dev_put(self.cmp_b)
        try:
            got = (c.first_diff(da, db, len(self.cmp_a)), c.first_diff(da, da, len(self.cmp_a)), c.first_diff(da, db, self.cmp_at))
        finally:
            c.dev_free(da); c.dev_free(db)
        assert got == (self.cmp_at, len(self.cmp_a), self.cmp_at), got
        return got

    def decode_rows(self, c):
        n, ml, B, Q, lens = self.rows_want
        gn, gml, gb, gq, gl = c.decode_rows_bytes(self.want)
        assert (gn, gml) == (n, ml), "decode_rows: %r rows / longest for %r" % ((gn, gml), (n, ml))
        for what, got, want in (("lengths", gl, lens), ("bases", gb, B), ("qualities", gq, Q)):
            assert np.array_equal(got, want), "decode_rows: %s differ, first in row %d" % (what, int(np.nonzero((got != want).reshape(n, -1).any(axis=1))[0][0]))
        return gn, gml, gb.tobytes(), gq.tobytes(), gl.tobytes()

    def decode_names(self, c):
        return tuple(self.mod["N"].check(c, self.want, want=self.names_want))     # (context-owned names and offsets, fetched inside check: before the next call)

    def text_rows(self, c):
        r, B, Q, lens, names = self.mod["T"].call(c, self.fq1, self.fq2, self.paired, recs=self.recs, extra="x16")
        return (int(r.n_rows), int(r.consumed1), int(r.consumed2)), B.tobytes(), Q.tobytes(), lens.tobytes(), tuple(names)

    def select_rows(self, c):
        return tuple(self.mod["S"].call(c, *self.rows, row_len="x16", **self.sel)[5])

    def judge_rows(self, c):
        J, W = self.mod["J"], self.mod["W"]; dev = W.DevRows(c, *self.j_rows)
        try:
            out, summ, raw = J.run(c, dev, self.j_crit, False)
        finally:
            dev.free()
        J.compare(out, summ, self.j_want, "calls circuit:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def adapter_rows(self, c):
        A, W = self.mod["A"], self.mod["W"]; B, lens = self.a_rows; dev = W.DevRows(c, B, None, lens)
        try:
            out, summ, raw = A.run(c, dev, self.a_crit, True)
        finally:
            dev.free()
        A.compare(out, summ, self.a_want, "calls circuit:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def merge_rows(self, c):
        return tuple(self.mod["M"].call(c, *self.m_rows, False, row_len="x16", paths=(None,), e=self.m_want)[3])

    def rows_to_text(self, c):
        got = c.rows_to_text_bytes(*self.rows, paired=self.paired)               # (context-owned texts, copied out inside: before the next call)
        assert got == (self.fq1, self.fq2), text_diff(got[0], self.fq1) or text_diff(got[1], self.fq2)
        return got

    def encode_rows(self, c):
        c.clearHeader()
        got = c.encode_rows_bytes(*self.rows, paired=self.paired, chunk_bases=self.cb, **E.nolb_args(self.fq1, self.fq2, self.paired))
        assert got == self.want, image_diff(got, self.want)
        return got


_CALLS = None


def calls():
    global _CALLS
    if _CALLS is None:
        _CALLS = Calls()
    return _CALLS


def first_results(make_codec):
    """{kind: what the call gives first on a fresh context} - each checked against its host reference inside the call"""
    out = {}
    for kind in CALL_KINDS:
        c = make_codec()
        try:
            out[kind] = getattr(calls(), kind)(c)
        finally:
            c.close()
    return out


def walk_calls(codec, first, seq, start=0, stop=None, prev=None):
    stop = len(seq) if stop is None else stop
    bad = []
    for i in range(start, stop):
        kind = CALL_KINDS[seq[i]]
        try:
            got = getattr(calls(), kind)(codec)
            if got != first[kind]:
                bad.append("step %d: %s behind %s equals its reference but not its own first result" % (i, kind, prev or "a fresh context"))
        except AssertionError as e:
            bad.append("step %d: %s behind %s: %s" % (i, kind, prev or "a fresh context", str(e)[:300]))
        prev = kind
    assert not bad, "%d of %d calls differ:\n%s" % (len(bad), stop - start, "\n".join(bad[:12]))
    return prev


# ---------------------------------------------------------------- state whose loss costs time, not bytes
def check_mixed_lengths_end_with_the_file(make_codec):
    """rfq_ctx::mixed_lengths (the prefix scans up front, no index without a read-back) is reset by new_file(): a uniform file encoded behind a file of mixed lengths
    is indexed without the read-back again.  A bit that stays up gives the same bytes by the slower route - no circuit can see it, the `lazy_index` stage can."""
    c = make_codec()
    try:
        for name in ("se150_big", "se_var", "se150_big", "three_records", "se150_big"):
            inp = by_name(name)
            msg = encode_step(c, inp)
            assert not msg, (name, msg)
            marks = {n for n, _ in c.timings()}
        assert "lazy_index" in marks, sorted(marks)
    finally:
        c.close()
