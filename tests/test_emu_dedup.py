"""CPU: rfq_dedup_rows - rows to a keep byte that leaves one unit of every class of identical units, the representative and the size of every class, a histogram
and a summary - under the SIMT interpreter, against a Python dict from key bytes to members (tests/_dedup.py).  The GPU twin is tests/test_gpu_dedup.py (it adds
the contention test: the interpreter runs a workgroup's lanes one after the other and cannot show a race); tools/dedup_asan.sh runs the good shapes and the
refusals through a stand-alone AddressSanitizer + UBSan program of the same sources."""
import pytest

import _dedup as D
import _engine as E


def make_codec():
    from repaq_amd import RfqCodec
    return RfqCodec(device=0, library=E.build_emu())


@pytest.fixture(scope="module")
def codec():
    c = make_codec()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_back_to_default(codec):
    yield
    E.reset_options(codec)


# ---- 1: planted classes
@pytest.mark.parametrize("pairs", [False, True], ids=["rows", "pairs"])
@pytest.mark.parametrize("row_len", D.ROW_LENS)
def test_planted_classes(codec, row_len, pairs):
    D.check_planted(codec, row_len, pairs)


# ---- 2: near misses
def test_one_byte_changed_at_every_position(codec):
    D.check_every_position(codec)


def test_lengths_padding_case_and_empty_rows(codec):
    D.check_lengths_and_padding(codec)


def test_key_len(codec):
    D.check_key_len(codec)


def test_pairs_are_keyed_mate_by_mate(codec):
    D.check_pairs(codec)


# ---- 3: best quality
def test_best_quality(codec):
    D.check_best_quality(codec)


# ---- 4: candidates
def test_candidates(codec):
    D.check_candidates(codec)


# ---- 5: shapes and outputs
def test_shapes_and_outputs(codec):
    D.check_shapes_and_outputs(codec)


# ---- 6: state
def test_nothing_is_left_of_an_earlier_table(codec):
    D.check_state(codec, make_codec)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    D.check_host_refusals(codec)


@pytest.mark.parametrize("label", D.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    D.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    D.check_option(codec, E.reset_options)


# ---- 8: text -> judge -> dedup -> select -> text
def test_text_judge_dedup_select_text(codec):
    D.check_composition(codec)


# ---- 12: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", [x for x in D.W.WALK_IDS if "general" not in x])
def test_walk_seams(codec, case):
    D.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    D.check_walk_bad_length(codec)
