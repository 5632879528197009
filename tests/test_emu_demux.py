"""CPU: rfq_demux_rows - rows against one or two sets of barcodes to a sample per unit, the reason where there is none, the keep byte and start rfq_select_rows takes
and a count per sample - under the SIMT interpreter, against a plain Python loop over units, barcodes and positions (tests/_demux.py).  The GPU twin is
tests/test_gpu_demux.py (it adds the composition with the tensors); tools/demux_asan.sh runs good shapes and
refusals through a stand-alone AddressSanitizer + UBSan program of the same sources."""
import pytest

import _demux as D
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


# ---- 1: every barcode at every distance (6: on both formulations, equal bytes)
@pytest.mark.parametrize("ln", D.PLANT_LENS)
def test_every_barcode_exact_one_mismatch_n_and_lower_case(codec, ln):
    D.check_every_distance(codec, ln)


# ---- 2: window seams
@pytest.mark.parametrize("off", D.SEAM_OFFS)
def test_windows_across_group_row_and_buffer_seams(codec, off):
    D.check_seams(codec, off)


# ---- 3: ties and deltas
def test_ties_deltas_one_barcode_and_4096(codec):
    D.check_ties(codec)


# ---- 4: pairs
def test_pairs_two_sets_sheet_every_reason_alone_masked_mates(codec):
    D.check_pairs(codec)


# ---- 5: the walk
@pytest.mark.parametrize("case", D.WALK_IDS)
def test_walk_seams(codec, case):
    D.check_walk(codec, case)


def test_walk_bad_length_in_the_last_row(codec):
    D.check_walk_bad_length(codec)


@pytest.mark.parametrize("cells", (8192, 8193))
def test_counts_in_lds_and_in_device_memory(codec, cells):
    D.check_counts_paths(codec, cells)


def test_the_largest_sets_and_count_table_the_lds_holds(codec):
    D.check_lds_max(codec)


def test_many_short_rows_take_several_steps(codec):
    D.check_many_rows(codec)


# ---- 6: the switch
def test_the_switch_is_listed_and_resets(codec):
    D.check_option(codec, E.reset_options)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    D.check_host_refusals(codec)


@pytest.mark.parametrize("label", D.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    D.check_device_refusal(codec, label)


# ---- 8: state
def test_a_demux_leaves_other_calls_alone_and_sets_of_any_size_follow_each_other(codec):
    D.check_state(codec)
