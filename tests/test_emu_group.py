"""CPU: rfq_group_rows - rfq_select_rows with the kept rows grouped by a bin per unit in one pass: a stable sort of the kept units by bin, the first output row of
every bin - under the SIMT interpreter, against a numpy / Python model and, bin by bin, against rfq_select_rows of the same library under the bin's mask
(tests/_group.py).  The sort works in tiles of GR_TILE = 2048 elements.  The GPU twin is tests/test_gpu_group.py (it adds the composition with the tensors);
tools/group_asan.sh runs good shapes and refusals through a stand-alone AddressSanitizer + UBSan program of the same sources."""
import pytest

import _engine as E
import _group as G


def make_codec():
    from repaq_amd import RfqCodec
    return RfqCodec(device=0, library=E.build_emu())


@pytest.fixture(scope="module")
def codec():
    c = make_codec()
    yield c
    c.close()


# ---- 1: unit counts
@pytest.mark.parametrize("units", G.UNITS)
def test_unit_counts_around_a_wave_a_step_and_a_tile(codec, units):
    G.check_units(codec, units)


def test_many_units_take_many_workgroups(codec):
    G.check_many_units(codec)


# ---- 2: total bins
@pytest.mark.parametrize("total", G.TOTALS)
def test_total_bins_one_pass_two_passes_and_the_limits(codec, total):
    G.check_totals(codec, total)


# ---- 3: bin patterns
@pytest.mark.parametrize("pattern", G.PATTERN_IDS)
def test_bin_patterns(codec, pattern):
    G.check_pattern(codec, pattern)


# ---- 4: the rest bin
def test_rest_bin_or_dropped_with_and_without_negative_bins(codec):
    G.check_rest(codec)


# ---- 5: pairs
def test_pairs_stay_adjacent_and_fall_with_their_mate(codec):
    G.check_pairs(codec)


# ---- 6: names
def test_rows_without_names_empty_names_and_a_long_name(codec):
    G.check_names(codec)


# ---- 7: layout, no rows left, partial outputs, determinism
def test_unaligned_and_aligned_row_buffers(codec):
    G.check_layout(codec)


def test_nothing_kept_writes_one_offset_and_zero_bin_offsets(codec):
    G.check_nothing_kept(codec)


def test_partial_outputs_and_bin_offsets_alone(codec):
    G.check_partial_outputs(codec)


def test_the_same_call_twice_writes_the_same_bytes(codec):
    G.check_same_bytes_twice(codec)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    G.check_host_refusals(codec)


def test_short_caps_are_nospace_and_nothing_is_written(codec):
    G.check_short_caps(codec)


@pytest.mark.parametrize("label", G.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    G.check_device_refusal(codec, label)


def test_a_bad_bin_beside_selects_device_refusals(codec):
    G.check_device_refusals_together(codec)


# ---- 9: state
def test_scratch_at_other_sizes_other_calls_unchanged_good_after_refused(codec):
    G.check_state(codec)
