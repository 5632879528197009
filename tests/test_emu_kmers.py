"""CPU: rfq_kmers_init, rfq_kmers_rows and rfq_kmers_read - rows to a caller-owned table of canonical k-mers with counts that adds up across calls, and the table
to its spectrum, its (value, count) list and a screen index - under the SIMT interpreter, against a collections.Counter made by a plain loop over the positions
(tests/_kmers.py).  The GPU twin is tests/test_gpu_kmers.py (it adds the repeated runs of the hot values, the many-rows walk and the tensors: the interpreter cannot
show a race that needs thousands of lanes in flight); tools/kmers_asan.sh runs the good shapes and the refusals through a stand-alone AddressSanitizer + UBSan
program of the same sources."""
import pytest

import _engine as E
import _kmers as K


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
@pytest.mark.parametrize("k", K.KS)
def test_a_planted_kmer_at_every_position(codec, k):
    K.check_every_position(codec, k)


# ---- 2: validity
def test_other_bytes_short_rows_padding_and_a_palindrome(codec):
    K.check_validity(codec)


# ---- 3: seams
@pytest.mark.parametrize("row_len", K.S.SEAM_IDS)
def test_kmers_across_lane_kernel_and_tile_seams(codec, row_len):
    K.check_seams(codec, row_len)


@pytest.mark.parametrize("case", K.W.WALK_IDS)
def test_walk_seams(codec, case):
    K.check_walk(codec, case)


def test_walk_bad_length_in_the_last_row(codec):
    K.check_walk_bad_length(codec)


# ---- 4: adding up
def test_calls_add_up_in_any_order_masks_cut_lengths_and_the_screens_kmers(codec):
    K.check_adding_up(codec)


# ---- 5: hot values
def test_hot_values(codec):
    K.check_hot(codec, twice=False)


# ---- 6: formulations
def test_default_general_direct_and_collide_agree(codec):
    K.check_formulations(codec)


def test_the_switch_is_listed_and_resets(codec):
    K.check_option(codec, E.reset_options)


# ---- 7: the read
def test_read_selection_spectrum_room_and_the_index(codec):
    K.check_read(codec)


# ---- 8: a table that is full
def test_a_full_table_is_refused_marked_and_formatted_again(codec):
    K.check_full(codec)


# ---- 9: refusals
def test_init_refused(codec):
    K.check_init_refusals(codec)


def test_rows_and_read_refused_on_the_host(codec):
    K.check_host_refusals(codec)


def test_a_table_that_is_none_and_a_table_of_garbage(codec):
    K.check_bad_table(codec)


@pytest.mark.parametrize("label", K.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    K.check_device_refusal(codec, label)


# ---- 10: state
def test_a_count_leaves_other_calls_alone(codec):
    K.check_state(codec)
