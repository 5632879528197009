"""CPU: rfq_screen_build and rfq_screen_rows - reference sequences to an exact set of canonical k-mers, rows to their k-mers, their hits and a keep byte - under
the SIMT interpreter, against a Python set of canonical ints and a plain loop over the positions (tests/_screen.py).  The GPU twin is tests/test_gpu_screen.py (it
adds the contention test of the build: the interpreter cannot show a race that needs thousands of lanes in flight); tools/screen_asan.sh runs the good shapes and the
refusals through a stand-alone AddressSanitizer + UBSan program of the same sources."""
import pytest

import _engine as E
import _screen as S


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


# ---- 1: every position, every k
@pytest.mark.parametrize("k", S.KS)
def test_a_reference_kmer_at_every_position(codec, k):
    S.check_every_position(codec, k)


# ---- 2: validity
def test_other_bytes_short_rows_padding_and_a_palindrome(codec):
    S.check_validity(codec)


# ---- 3: seams
@pytest.mark.parametrize("row_len", S.SEAM_IDS)
def test_hits_across_lane_kernel_and_tile_seams(codec, row_len):
    S.check_seams(codec, row_len)


@pytest.mark.parametrize("case", S.W.WALK_IDS)
def test_walk_seams(codec, case):
    S.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    S.check_walk_bad_length(codec)


# ---- 4: the verdict
def test_verdict_boundaries_modes_pairs_candidates_outputs(codec):
    S.check_verdict(codec)


# ---- 5: the set
def test_the_set_of_a_reference_list(codec):
    S.check_set(codec)


def test_lds_and_device_memory_placement_agree(codec):
    S.check_placements(codec)


# ---- 6: refusals
def test_build_refused(codec):
    S.check_build_refusals(codec)


def test_rows_refused_on_the_host(codec):
    S.check_host_refusals(codec)


def test_an_index_that_is_none_and_an_index_that_is_full(codec):
    S.check_bad_index(codec)


@pytest.mark.parametrize("label", S.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    S.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    S.check_option(codec, E.reset_options)


# ---- 7: state and composition
def test_a_screen_leaves_other_calls_alone(codec):
    S.check_state(codec)


def test_text_adapter_judge_screen_dedup_select_text(codec):
    S.check_composition(codec)
