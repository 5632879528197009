"""CPU (the SIMT interpreter build, tests/emu): what a context carries from call to call.  Every other test makes a result once, on a context whose earlier calls
are whatever the collection order gave; here ONE context lives through a sequence in which every input follows every other one exactly once (tests/_history.py:
an Eulerian circuit over a dozen texts, each there for one piece of rfq_ctx state, each proven to reach that state by its stage markers on a fresh context or, where no stage shows it, by the oracle's image), and
every image and text is the oracle's.  The same over the nineteen KINDS of call.  Then the refusals: every refusing input (and refusing kind of call) behind and in
front of every good one and every other refusing one, each refusal the oracle's; and a small batch behind a large one for every rows call.  The interpreter runs the
host code the product runs - the bookkeeping between calls is host code - but no two workgroups at once: races are tests/test_gpu_history.py's.

A circuit costs about 0.2 s per call here, so each is cut into PARTS slices (the two circuits over the kinds of call, which have grown with the kinds, into
CALLS_PARTS) that share one context through a module fixture and run in order."""
import pytest

import _engine as E
import _history as H

PARTS = 4
CALLS_PARTS = 8                                 # (362 and 1009 calls: no slice longer than the longest of the four that 197 and 481 calls were cut into)
NAMES = [i.name for i in H.inputs()]


@pytest.fixture(scope="module")
def make():
    from repaq_amd import RfqCodec
    lib = E.build_emu(); made = []

    def make_codec():
        c = RfqCodec(device=0, library=lib)
        assert "simt-emulation" in c.version()
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


@pytest.fixture(scope="module")
def lives(make):
    """{circuit: [the context that lives through it, what it did last]}"""
    book = {}

    def life(name):
        if name not in book:
            book[name] = [make(), None]
        return book[name]
    return life


def _slice(n, part, parts=PARTS):
    return n * part // parts, n * (part + 1) // parts


@pytest.mark.parametrize("k", [1, 2, 5, 12, 13])
def test_euler_visits_every_ordered_pair_once(k):
    seq = H.euler(k)                                                         # (asserts length and pair count itself)
    assert len(seq) == k * k + 1 and set(seq) == set(range(k))
    assert sorted(zip(seq, seq[1:])) == [(a, b) for a in range(k) for b in range(k)]


def test_the_inputs_are_the_dozen_the_circuits_need():
    ins = H.inputs()
    assert len(ins) == 13 and len(set(NAMES)) == 13
    # (a marker rule that goes missing fails here: first encode, decode, second encode)
    assert {i.name: (i.enc_mark, i.dec_mark, i.enc2_mark) for i in ins} == {
        "pe150": (("mirror_index", "!mirror_fallback"), (), ("mirror_index", "lazy_index")),
        "pe_unmirrored": (("mirror_fallback", "!mirror_index"), (), ()),
        "se_var": ((), (), ()),                                               # (mixed lengths: the chunk flags of the oracle's image, _history.inputs)
        "bgi_q40": (("!quality_masks",), (), ()),
        "four_quals": (("retry_room", "quality_masks"), (), ()),
        "rare_quals": (("quality_masks",), (), ()),                           # (+ the header's table and the counts per chunk, _history._rare_planes_are_reached)
        "long_names": ((), ("emit", "emit_expanded"), ()),
        "crlf": ((), (), ("!lazy_index",)),
        "empty_line": ((), (), ("!lazy_index",)),
        "interleaved": ((), (), ("lazy_index",)),
        "se150_big": ((), (), ("lazy_index",)),
        "three_records": ((), (), ("lazy_index",)),
        "lowercase_late": (("quality_masks",), (), ()),                       # (the oracle encodes a lower-case base behind chunk 0: _history.inputs)
    }
    assert len(H.by_name("three_records").fq1.split(b"\n")) == 13


@pytest.mark.parametrize("name", NAMES)
def test_input_reaches_its_state_on_a_fresh_context(fresh, name):
    H.check_markers(fresh, H.by_name(name))


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("kind", ["encode", "decode", "mixed"])
def test_every_input_behind_every_other(lives, kind, part):
    seq = H.euler(len(NAMES)); life = lives(kind)
    a, b = _slice(len(seq), part)
    try:
        life[1] = H.walk(life[0], seq, H.KINDS[kind], a, b, state=life[1])
    except AssertionError:
        life[1] = {"prev": "a failed slice", "enc": "a failed slice", "dec": "a failed slice"}
        raise


@pytest.mark.parametrize("name,other", [("se_var", "bgi_q40"), ("rare_quals", "four_quals"), ("four_quals", "long_names"), ("se150_big", "pe_unmirrored")])
def test_one_file_in_two_batches_with_a_decode_between(lives, name, other):
    inp = H.by_name(name)
    got = H.check_two_batches(lives("two_batches")[0], inp, H.by_name(other))
    assert got == inp.want, H.image_diff(got, inp.want)


def test_mixed_lengths_end_with_the_file(fresh):
    H.check_mixed_lengths_end_with_the_file(fresh)


# ---------------------------------------------------------------- refusals in sequence on a context that lives on
@pytest.mark.parametrize("g,r", [(1, 1), (3, 2), (13, 9), (13, 15), (0, 4)])
def test_circuit_walks_every_edge_of_the_refusal_digraph_once(g, r):
    edges = H.refusal_edges(g, r)
    seq = H.circuit(range(g + r), edges)                                     # (asserts closure and every edge once itself)
    assert len(edges) == 2 * g * r + r * r and len(seq) == len(edges) + 1 and seq[0] == seq[-1]
    assert sorted(zip(seq, seq[1:])) == sorted(edges) and not [(a, b) for a, b in zip(seq, seq[1:]) if a < g and b < g]


def test_circuit_refuses_a_digraph_without_one():
    for edges in ([(0, 1)], [(0, 1), (1, 0), (2, 2)], [(0, 1), (0, 1), (1, 0), (1, 0)]):      # (not closed; not connected; an edge twice)
        with pytest.raises(AssertionError):
            H.circuit(range(3), edges)


def test_the_refusing_inputs_are_the_ones_the_circuits_need():
    """refusals() itself asserts, for every entry, that the oracle takes the unmutated text (image) and refuses the mutated one, and that a late mutation lies behind
    two chunks; here: which there are, and that each message is the reference's"""
    ref = H.refusals()
    assert [(r.name, r.kind, r.codes) for r in ref if r.kind == "enc"] == [
        ("coord_late_masks", "enc", (-5,)), ("coord_late_pe", "enc", (-5,)), ("coord_late_list", "enc", (-5,)), ("lowercase_chunk0", "enc", (-5,)),
        ("iupac_chunk0_long", "enc", (-5,)), ("bad_qual_chunk0", "enc", (-5,)), ("qual_short_late", "enc", (-7,)), ("nospace", "enc", (-8,)), ("qual_overflow", "enc", (-7,))]
    assert [r.name for r in ref if r.kind == "dec"] == ["cut_last_chunk", "scribbled_lengths", "scribbled_quality", "lying_index", "se_split", "text_nospace"]
    said = {r.name: (r.message or r.phrase or "").split("\n")[0] for r in ref}
    coord = "The X/Y coordinate cannot be larger than 2M, but we get: 2097152"
    assert (said["coord_late_masks"], said["coord_late_pe"], said["coord_late_list"]) == (coord,) * 3
    assert said["lowercase_chunk0"] == "repaq doesn't support FASTQ with lowercase bases (a/t/c/g)"
    assert said["iupac_chunk0_long"] == "repaq only supports FASTQ with uppercase bases (A/T/C/G/N)"
    assert said["bad_qual_chunk0"] == "bad quality value: -123"
    assert said["se_split"] == "The input RFQ file was encoded by single-end FASTQ, you should not specify <out2>"
    assert H.MUTANT_LABELS["lying_index"] == ("pe150", "index0") and H.refusal("lying_index").text == H.by_name("pe150").text


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("kind", ["encode", "decode", "mixed"])
def test_every_refusal_behind_and_in_front_of_every_input(lives, kind, part):
    nodes, seq, g, r = H.refusal_circuit(kind)
    assert g == 13 and r == {"encode": 9, "decode": 6, "mixed": 15}[kind] and len(seq) == 2 * g * r + r * r + 1
    life = lives("refusals " + kind)
    a, b = _slice(len(seq), part)
    try:
        life[1] = H.walk(life[0], seq, H.KINDS[kind], a, b, state=life[1], nodes=nodes)
    except AssertionError:
        life[1] = {"prev": "a failed slice", "enc": "a failed slice", "dec": "a failed slice"}
        raise


def test_no_refusal_costs_the_context_its_fast_path(lives):
    """on the context that has been through the encode circuit of refusals (a fresh one when this test runs alone)"""
    H.check_fast_path_kept(lives("refusals encode")[0])


def test_the_header_made_survives_a_refusal_at_the_last_exit(fresh):
    H.check_header_survives_refusal(fresh())


@pytest.fixture(scope="module")
def first(make):
    return H.first_results(make)


@pytest.mark.parametrize("part", range(CALLS_PARTS))
def test_every_kind_of_call_behind_every_other(lives, first, part):
    seq = H.euler(len(H.CALL_KINDS)); life = lives("calls")
    assert len(H.CALL_KINDS) == 19 and len(seq) == 362
    a, b = _slice(len(seq), part, CALLS_PARTS)
    life[1] = H.walk_calls(life[0], first, seq, a, b, prev=life[1])


@pytest.mark.parametrize("part", range(CALLS_PARTS))
def test_every_refusing_kind_of_call_behind_and_in_front_of_every_kind(lives, first, part):
    kinds, seq = H.calls_refusal_circuit(); life = lives("refusing calls")
    g, r = len(H.CALL_KINDS), len(H.REFUSING_CALL_KINDS)
    assert (g, r) == (19, 18) and len(kinds) == 37 and len(seq) == 2 * g * r + r * r + 1 == 1009
    a, b = _slice(len(seq), part, CALLS_PARTS)
    life[1] = H.walk_calls(life[0], first, seq, a, b, prev=life[1], kinds=kinds)


@pytest.mark.parametrize("kind", H.NOTHING_LEFT_CALLS)
def test_nothing_is_left_of_a_larger_call(lives, make, kind):
    assert len(H.NOTHING_LEFT_CALLS) == 15
    H.check_nothing_left(lives("nothing left")[0], make, kind)
