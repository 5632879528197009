"""CPU (the SIMT interpreter build, tests/emu): what a context carries from call to call.  Every other test makes a result once, on a context whose earlier calls
are whatever the collection order gave; here ONE context lives through a sequence in which every input follows every other one exactly once (tests/_history.py:
an Eulerian circuit over a dozen texts, each there for one piece of rfq_ctx state, each proven to reach that state by its stage markers on a fresh context or, where no stage shows it, by the oracle's image), and
every image and text is the oracle's.  The same over the thirteen KINDS of call.  The interpreter runs the host code the product runs - the bookkeeping between
calls is host code - but no two workgroups at once: races are tests/test_gpu_history.py's.

A circuit of 145 calls costs about 0.2 s per call here, so each is cut into PARTS slices that share one context through a module fixture and run in order."""
import pytest

import _engine as E
import _history as H

PARTS = 4
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


def _slice(n, part):
    return n * part // PARTS, n * (part + 1) // PARTS


@pytest.mark.parametrize("k", [1, 2, 5, 12, 13])
def test_euler_visits_every_ordered_pair_once(k):
    seq = H.euler(k)                                                         # (asserts length and pair count itself)
    assert len(seq) == k * k + 1 and set(seq) == set(range(k))
    assert sorted(zip(seq, seq[1:])) == [(a, b) for a in range(k) for b in range(k)]


def test_the_inputs_are_the_dozen_the_circuits_need():
    ins = H.inputs()
    assert len(ins) == 12 and len(set(NAMES)) == 12
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


@pytest.fixture(scope="module")
def first(make):
    return H.first_results(make)


@pytest.mark.parametrize("part", range(PARTS))
def test_every_kind_of_call_behind_every_other(lives, first, part):
    seq = H.euler(len(H.CALL_KINDS)); life = lives("calls")
    assert len(H.CALL_KINDS) == 13 and len(seq) == 170
    a, b = _slice(len(seq), part)
    life[1] = H.walk_calls(life[0], first, seq, a, b, prev=life[1])
