"""GPU (MI355X, the product library): three things no test that makes each result once can see.

A. History.  One context lives through a sequence in which every input follows every other one exactly once (tests/_history.py), encoding, decoding, both in turn,
   one file in two batches with another file's decode between them, and every KIND of call behind every other kind; every result is the oracle's / its host loop's.
   A': the same with refusals in the sequence - every refusing input and refusing kind of call behind and in front of every good one and every other refusing one -
   and a small batch behind a large one for every rows call.
B. Repeats.  Inputs with many more workgroups than the device has compute units, each encoded and decoded R = 16 times on one context under the formulations that
   move the communication between workgroups (the look-back of k_line_index, the plane words at tile edges of k_gather2, the segment counters, the chunk walk's
   atomicMin, the list chain).  Every result is compared ON the device (rfq_compare_bytes) with the oracle's, uploaded once.
C. Contexts side by side.  include/rfq_hip.h: "distinct contexts may be used concurrently" - two and three contexts on device 0, a host thread each, walk A's
   sequences (the inputs', and the one over the kinds of call) from different offsets; per-context switches stay per context; two contexts run B's largest
   input at the same time (the host queue's configuration).

B and C can SHOW a race - a mismatch names repeat, offset, chunk, section and stages - and can never rule one out: sixteen equal results are sixteen equal results.
R is a condition of the test, not a measurement of anything.  No loop here runs until something differs or goes on after a difference."""
import functools
import json
import os
import subprocess
import sys

import pytest

import _engine as E
import _history as H
import _oracle as O
import _sections

pytestmark = pytest.mark.gpu
NAMES = [i.name for i in H.inputs()]
R = 16
CB = 100_000
MIN_CHUNKS = 100                                # B: many more workgroups than the 256 compute units


@pytest.fixture(scope="module")
def make():
    import torch
    assert torch.cuda.is_available()
    from repaq_amd import RfqCodec
    made = []

    def make_codec():
        c = RfqCodec(device=0, library=E.PRODUCT_LIB)
        assert "gfx950" in c.version()
        E.reset_options(c)                      # (whatever the environment says)
        made.append(c)
        return c
    yield make_codec
    for c in made:
        c.close()


@pytest.fixture()
def fresh(make):
    """contexts that end with the test"""
    mine = []

    def make_codec():
        mine.append(make())
        return mine[-1]
    yield make_codec
    for c in mine:
        c.close()


# ---------------------------------------------------------------- A: every input after every other
@pytest.mark.parametrize("name", NAMES)
def test_input_reaches_its_state_on_a_fresh_context(fresh, name):
    H.check_markers(fresh, H.by_name(name))


@pytest.mark.parametrize("kind", ["encode", "decode", "mixed"])
def test_every_input_behind_every_other(fresh, kind):
    seq = H.euler(len(NAMES))
    assert len(seq) == 170
    H.walk(fresh(), seq, H.KINDS[kind])


@pytest.mark.parametrize("name,other", [("se_var", "bgi_q40"), ("rare_quals", "four_quals"), ("four_quals", "long_names"), ("se150_big", "pe_unmirrored")])
def test_one_file_in_two_batches_with_a_decode_between(fresh, name, other):
    inp = H.by_name(name)
    got = H.check_two_batches(fresh(), inp, H.by_name(other))
    assert got == inp.want, H.image_diff(got, inp.want)


def test_mixed_lengths_end_with_the_file(fresh):
    H.check_mixed_lengths_end_with_the_file(fresh)


def test_every_kind_of_call_behind_every_other(fresh):
    seq = H.euler(len(H.CALL_KINDS))
    assert len(H.CALL_KINDS) == 19 and len(seq) == 362
    H.walk_calls(fresh(), H.first_results(fresh), seq)


# ---------------------------------------------------------------- A': refusals in sequence on a context that lives on
# Every refusing input of tests/_history.py behind and in front of every good one and every other refusing one (refusal_circuit).  The circuits that hold decode
# mutants run in a CHILD process, like tests/test_gpu_rows_hostile.py: a device fault ends the process, and the test says so.
HERE = os.path.dirname(os.path.abspath(__file__))
REFUSAL_CHILD = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import _engine as E, _history as H
from repaq_amd import RfqCodec
kind = sys.argv[1]
c = RfqCodec(device=0, library=E.PRODUCT_LIB)
assert "gfx950" in c.version()
E.reset_options(c)
nodes, seq, g, r = H.refusal_circuit(kind)
out = {"g": g, "r": r, "steps": len(seq), "failed": ""}
try:
    H.walk(c, seq, H.KINDS[kind], nodes=nodes)
except AssertionError as e:
    out["failed"] = str(e)
c.close()
print("SUMMARY " + json.dumps(out))
""" % (HERE, os.path.join(HERE, "golden"), os.path.dirname(HERE))


def test_every_refusal_behind_and_in_front_of_every_input_encode(fresh):
    nodes, seq, g, r = H.refusal_circuit("encode")
    assert (g, r) == (13, 9) and len(seq) == 2 * g * r + r * r + 1
    codec = fresh()
    H.walk(codec, seq, H.KINDS["encode"], nodes=nodes)
    H.check_fast_path_kept(codec)                                            # (no refusal costs the context its fast path for good)


@pytest.mark.parametrize("kind,r_want", [("decode", 6), ("mixed", 15)])
def test_every_refusal_behind_and_in_front_of_every_input(kind, r_want):
    r = subprocess.run([sys.executable, "-c", REFUSAL_CHILD, kind], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, "the child process ended with status %d (negative: a signal - a device fault aborts the process):\n%s" % (r.returncode, tail)
    line = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, tail
    s = json.loads(line[-1][8:])
    assert not s["failed"], s["failed"]
    assert (s["g"], s["r"]) == (13, r_want) and s["steps"] == 2 * 13 * r_want + r_want * r_want + 1, s


def test_the_header_made_survives_a_refusal_at_the_last_exit(fresh):
    H.check_header_survives_refusal(fresh())


@pytest.mark.parametrize("kind", H.NOTHING_LEFT_CALLS)
def test_nothing_is_left_of_a_larger_call(fresh, kind):
    assert len(H.NOTHING_LEFT_CALLS) == 15
    H.check_nothing_left(fresh(), fresh, kind)


CALLS_CHILD = r"""
import json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import _engine as E, _history as H
from repaq_amd import RfqCodec
made = []
def make():
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    E.reset_options(c)
    made.append(c)
    return c
kinds, seq = H.calls_refusal_circuit()
out = {"g": len(H.CALL_KINDS), "r": len(H.REFUSING_CALL_KINDS), "steps": len(seq), "failed": ""}
try:
    H.walk_calls(make(), H.first_results(make), seq, kinds=kinds)
except AssertionError as e:
    out["failed"] = str(e)
for c in made:
    c.close()
print("SUMMARY " + json.dumps(out))
""" % (HERE, os.path.join(HERE, "golden"), os.path.dirname(HERE))


def test_every_refusing_kind_of_call_behind_and_in_front_of_every_kind():
    r = subprocess.run([sys.executable, "-c", CALLS_CHILD], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    tail = (r.stdout[-1500:] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, "the child process ended with status %d (negative: a signal - a device fault aborts the process):\n%s" % (r.returncode, tail)
    line = [l for l in r.stdout.splitlines() if l.startswith("SUMMARY ")]
    assert line, tail
    s = json.loads(line[-1][8:])
    assert not s["failed"], s["failed"]
    assert (s["g"], s["r"], s["steps"]) == (19, 18, 2 * 19 * 18 + 18 * 18 + 1) and s["steps"] == 1009, s


# ---------------------------------------------------------------- B: the same result every time
BIG = {"pe150": (O.NOVA_PE150, 150_000, 51, {}, O.PE_TWO_FILES), "se_var": (O.SE_VAR, 200_000, 52, {}, O.SE),
       "bgi_q40": (O.BGI_PE100, 100_000, 53, dict(n_quals=40), O.PE_TWO_FILES)}
ENC_FORMS = ["default", "idx_tiles4", "one_stream", "gather_old"]
DEC_FORMS = ["default", "gw_small", "pos_seg_1024", "no_spec"]


@functools.lru_cache(maxsize=None)
def big(name):
    """(fq1, fq2, paired, the oracle's image) - made once"""
    prof, reads, seed, kw, paired = BIG[name]
    fq1, fq2 = O.gen(prof, reads, seed=seed, **kw)
    want = O.encode_file(fq1, fq2, paired, CB)
    assert O.decode_file(want, paired == O.PE_TWO_FILES) == ((fq1, fq2) if paired == O.PE_TWO_FILES else fq1)
    return fq1, fq2, paired, want


class Uploaded:
    """an input of B on the device, for one context: the texts, the oracle's image, output buffers for the decoder"""
    def __init__(self, codec, name):
        self.codec, self.name = codec, name
        self.fq1, self.fq2, self.paired, self.want = big(name)
        self.two = self.paired == O.PE_TWO_FILES
        self.d1 = codec.dev_put(self.fq1); self.d2 = codec.dev_put(self.fq2) if self.two else None
        self.d_want = codec.dev_put(self.want)
        self.cap1 = len(self.fq1) + 64; self.cap2 = len(self.fq2) + 64 if self.two else 0
        self.o1 = codec.dev_put(b"\0" * self.cap1); self.o2 = codec.dev_put(b"\0" * self.cap2) if self.two else None
        assert self.o1.value % 16 == 0 and (self.o2 is None or self.o2.value % 16 == 0)
        self.nolb = E.nolb_args(self.fq1, self.fq2, self.paired)

    def free(self):
        for p in (self.d1, self.d2, self.d_want, self.o1, self.o2):
            if p is not None:
                self.codec.dev_free(p)

    def encode_once(self, rep, of=R):
        """one encode, compared on the device; a mismatch raises with everything the cause can be read from"""
        c = self.codec
        c.clearHeader()
        r = c.encode(self.d1, len(self.fq1), self.d2, len(self.fq2) if self.two else 0, self.paired, CB, **self.nolb)
        n = min(r.rfq_len, len(self.want))
        at = c.first_diff(r.d_rfq, self.d_want, n)
        if r.rfq_len != len(self.want) or at != n:
            stages = [s for s, _ in c.timings()]
            chunk, section = H.where(self.want, at)
            raise AssertionError("%s, repeat %d of %d: %d bytes for %d, first difference at offset %d: chunk %s, section %s; stages %s" % (
                self.name, rep, of, r.rfq_len, len(self.want), at, chunk, section, stages))

    def decode_once(self, rep, of=R):
        c = self.codec
        r = c.decode(self.d_want, len(self.want), split_pe=self.two, d_out1=self.o1, cap1=self.cap1, d_out2=self.o2, cap2=self.cap2)
        for which, got, n_got, d_text, text in ((1, r.d_fq1, r.n1, self.d1, self.fq1),) + (((2, r.d_fq2, r.n2, self.d2, self.fq2),) if self.two else ()):
            n = min(n_got, len(text))
            at = c.first_diff(got, d_text, n)
            if n_got != len(text) or at != n:
                stages = [s for s, _ in c.timings()]
                rec = text[:at].count(b"\n") // 4                             # the record of this text; a chunk holds both mates' records
                _, chunks = _sections.parse(self.want); seen = 0; chunk = "?"
                for k, ch in enumerate(chunks):
                    seen += ch.reads // (2 if self.two else 1)
                    if rec < seen:
                        chunk = k
                        break
                raise AssertionError("%s, repeat %d of %d: text %d has %d bytes for %d, first difference at offset %d: record %d, chunk %s; stages %s" % (
                    self.name, rep, of, which, n_got, len(text), at, rec, chunk, stages))


@pytest.fixture(scope="module")
def uploaded(make):
    """{input: Uploaded} on one context that lives through all of B"""
    codec = make(); book = {}; differed = []

    def get(name):
        assert not differed, "an earlier repeat test differed on this context (%s): nothing is run on it again" % differed[0]
        if name not in book:
            book[name] = Uploaded(codec, name)
        return book[name]
    get.differed = differed
    yield get
    for u in book.values():
        u.free()


@pytest.mark.parametrize("form", ENC_FORMS)
@pytest.mark.parametrize("name", sorted(BIG))
def test_encode_gives_the_same_image_every_time(uploaded, name, form):
    u = uploaded(name); opts, marker = E.ENC_FORMS[form]
    assert len(O.chunk_table(u.want)) - 1 >= MIN_CHUNKS
    with E.Options(u.codec, opts):
        try:
            for rep in range(R):
                u.encode_once(rep)                                           # (raises at the first difference: nothing runs behind it, in this test or a later one)
        except AssertionError:
            uploaded.differed.append("encode %s %s" % (name, form))
            raise
        E.marker_ok(u.codec, marker)


@pytest.mark.parametrize("form", DEC_FORMS)
@pytest.mark.parametrize("name", sorted(BIG))
def test_decode_gives_the_same_text_every_time(uploaded, name, form):
    u = uploaded(name); opts, marker = E.DEC_FORMS[form]
    with E.Options(u.codec, opts):
        try:
            for rep in range(R):
                u.decode_once(rep)
        except AssertionError:
            uploaded.differed.append("decode %s %s" % (name, form))
            raise
        E.marker_ok(u.codec, marker)


# ---------------------------------------------------------------- C: contexts side by side
def _rotated(seq, at):
    """the closed circuit, begun at step `at`"""
    return seq[at:] + seq[1:at + 1]


@pytest.mark.parametrize("n_threads", [2, 3])
def test_contexts_side_by_side_walk_the_circuit(fresh, n_threads):
    seq = H.euler(len(NAMES))
    kinds = [H.KINDS["encode"], H.KINDS["decode"], H.KINDS["mixed"]]
    codecs = [fresh() for _ in range(n_threads)]

    def job(i):
        mine = _rotated(seq, i * len(seq) // n_threads)
        assert len(mine) == len(seq) and set(zip(mine, mine[1:])) == set(zip(seq, seq[1:]))
        return lambda: H.walk(codecs[i], mine, kinds[i])
    H.run_threads([job(i) for i in range(n_threads)])


@pytest.fixture(scope="module")
def first(make):
    """what every kind of call gives first on a fresh context, made once for the walks side by side"""
    return H.first_results(make)


@pytest.mark.parametrize("n_threads", [2, 3])
def test_contexts_side_by_side_walk_the_calls_circuit(fresh, first, n_threads):
    """the kinds of call - the rows family with its device-wide tables (dedup's claims, the k-mer table's claims and 64-bit adds, the profile's adds) among
    them - on two and three contexts at the same time, each from another place of the circuit, all against one set of first results.  No refusing kinds: a
    fault in a thread could not be contained.  One walk per context"""
    seq = H.euler(len(H.CALL_KINDS))
    codecs = [fresh() for _ in range(n_threads)]

    def job(i):
        mine = _rotated(seq, i * len(seq) // n_threads)
        assert len(mine) == len(seq) and set(zip(mine, mine[1:])) == set(zip(seq, seq[1:]))
        return lambda: H.walk_calls(codecs[i], first, mine)
    H.run_threads([job(i) for i in range(n_threads)])


def test_a_context_of_refusals_beside_a_context_of_good_calls(fresh):
    """one context walks the encode circuit of refusals, one the circuit of good inputs from its middle, at the same time: a refusal's error path (the second stream
    joined, read-backs dropped) is the context's own"""
    nodes, rseq, g, r = H.refusal_circuit("encode")
    seq = H.euler(len(NAMES))
    refusing, good = fresh(), fresh()
    H.run_threads([lambda: H.walk(refusing, rseq, H.KINDS["encode"], nodes=nodes), lambda: H.walk(good, _rotated(seq, len(seq) // 2), H.KINDS["mixed"])])


def test_switches_stay_with_their_context(fresh):
    """one context on the byte-wise gather and one stream, one on the defaults, encoding the circuit at the same time: c->opt is the context's own"""
    seq = H.euler(len(NAMES))
    old, plain = fresh(), fresh()
    old.set_option("RFQ_GATHER", "old"); old.set_option("RFQ_STREAMS", "1")
    marks = {}

    def job(codec, tag, mine):
        def run():
            H.walk(codec, mine, H.KINDS["encode"])
            marks[tag] = {s for s, _ in codec.timings()}
        return run
    H.run_threads([job(old, "old", seq), job(plain, "plain", _rotated(seq, len(seq) // 2))])
    assert (old.get_option("RFQ_GATHER"), old.get_option("RFQ_STREAMS")) == ("old", "1")
    assert (plain.get_option("RFQ_GATHER"), plain.get_option("RFQ_STREAMS")) == ("", "")
    assert "gather_bytes" in marks["old"] and "gather_bytes" not in marks["plain"], marks


def test_two_contexts_overlap_on_the_device(fresh):
    """the host queue's configuration: two worker contexts, a host thread each, the same large input at the same time - 8 encodes each, then 8 decodes each"""
    ups = [Uploaded(fresh(), "pe150") for _ in range(2)]
    try:
        def enc(u):
            def run():
                for rep in range(8):
                    u.encode_once(rep, 8)
            return run

        def dec(u):
            def run():
                for rep in range(8):
                    u.decode_once(rep, 8)
            return run
        H.run_threads([enc(u) for u in ups])
        H.run_threads([dec(u) for u in ups])
    finally:
        for u in ups:
            u.free()
