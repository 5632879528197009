"""CPU: rfq_adapter_rows - rows to the length adapter removal leaves, the detector that cut, the pairs' insert sizes, a summary and an insert-size histogram - under
the SIMT interpreter, against plain loops over the shifts and positions on the host (tests/_adapter.py).  The GPU twin is tests/test_gpu_adapter.py;
tools/adapter_asan.sh runs the good shapes and the refusals through a stand-alone AddressSanitizer + UBSan program of the same sources (log:
profiles/r16_adapter_asan.txt)."""
import pytest

import _adapter as A
import _engine as E


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.build_emu())
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_back_to_default(codec):
    yield
    E.reset_options(codec)


# ---- 1: shapes
@pytest.mark.parametrize("row_len", A.ROW_LENS)
def test_shapes(codec, row_len):
    A.check_shapes(codec, row_len)


# ---- 2: every shift
@pytest.mark.parametrize("lengths", A.EVERY_SHIFT_IDS)
def test_every_shift(codec, lengths):
    A.check_every_shift(codec, lengths)


# ---- 3: thresholds at equality
def test_thresholds_at_equality(codec):
    A.check_thresholds(codec)


# ---- 4: the order of the shifts
def test_order_of_the_shifts(codec):
    A.check_order(codec)


# ---- 5: base classes
def test_base_classes(codec):
    A.check_classes(codec)


# ---- 6: the adapter at every position
@pytest.mark.parametrize("adapter_len", A.ADAPTER_LENS)
def test_adapter_at_every_position(codec, adapter_len):
    A.check_adapter_positions(codec, adapter_len)


# ---- 7: both detectors
def test_both_detectors(codec):
    A.check_both(codec)


# ---- 8: degenerate
def test_degenerate(codec):
    A.check_degenerate(codec)


# ---- 9: each output alone, none, twice the same, the histogram
def test_outputs_and_histogram(codec):
    A.check_outputs(codec)


# ---- 10: refusals
def test_refused_on_the_host(codec):
    A.check_host_refusals(codec)


@pytest.mark.parametrize("label", A.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    A.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    assert "RFQ_ADAPTER" in codec.option_names()
    codec.set_option("RFQ_ADAPTER", "general")
    assert codec.get_option("RFQ_ADAPTER") == "general"
    E.reset_options(codec)
    assert codec.get_option("RFQ_ADAPTER") == ""
    codec.set_option("RFQ_ADAPTER", "staged")
    from repaq_amd import RfqError
    with pytest.raises(RfqError):
        codec.set_option("RFQ_ADAPTER", "fast")


def test_stage_time_is_reported(codec):
    import numpy as np
    B, lens = A.random_pairs(4, 40, 1, codes=True)
    A.check(codec, B, lens, A.shape_criteria(40)[2][1], True, paths=(None,))
    assert [n for n, _ in codec.timings()] == ["adapter:rows"] and np.isfinite(codec.timings()[0][1])


# ---- 11: text -> adapter -> judge -> select -> text
def test_text_adapter_judge_select_text(codec):
    A.check_composition(codec)


# ---- 12: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", A.W.WALK_IDS)
def test_walk_seams(codec, case):
    A.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    A.check_walk_bad_length(codec)
