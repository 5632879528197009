"""CPU: rfq_judge_rows - rows to a keep byte, a window, a reason byte and four metrics per row and one QC summary - under the SIMT interpreter, against a plain
per-row loop on the host (tests/_judge.py).  The GPU twin is tests/test_gpu_judge.py; tools/judge_asan.sh runs the good shapes and the refusals through a
stand-alone AddressSanitizer + UBSan program of the same sources (log: profiles/r14_judge_asan.txt)."""
import pytest

import _engine as E
import _judge as J


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


# ---- 1: every step alone, then all together
@pytest.mark.parametrize("row_len", J.ROW_LENS)
def test_every_step_alone_and_all_together(codec, row_len):
    J.check_steps(codec, row_len)


# ---- 2: window seams
@pytest.mark.parametrize("cut_window", [1, 4, 300, 500])
@pytest.mark.parametrize("kind", ["front", "right", "tail"])
def test_window_at_every_position(codec, kind, cut_window):
    J.check_seams(codec, kind, cut_window, trim=0 if cut_window != 4 else 2)


@pytest.mark.parametrize("kind", ["front", "right", "tail"])
def test_window_of_1000_on_a_longer_row(codec, kind):
    J.check_seams(codec, kind, 1000, L=1500, step=41)


# ---- 3: poly-G
def test_poly_g(codec):
    J.check_poly_g(codec)


# ---- 4: every reason at equality
def test_every_reason_at_equality(codec):
    J.check_reasons(codec)


# ---- 5: empty and degenerate
def test_empty_and_degenerate(codec):
    J.check_degenerate(codec)


# ---- 6: a long row, naturally
def test_long_rows(codec):
    J.check_long_rows(codec)


# ---- 7 and 8: each output alone, none, the summary, twice the same
def test_outputs_and_summary(codec):
    J.check_outputs_and_summary(codec)


# ---- 9: refusals
def test_refused_on_the_host(codec):
    J.check_host_refusals(codec)


@pytest.mark.parametrize("label", J.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    J.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    assert "RFQ_JUDGE" in codec.option_names()
    codec.set_option("RFQ_JUDGE", "general")
    E.reset_options(codec)
    assert codec.get_option("RFQ_JUDGE") == ""
    from repaq_amd import RfqError
    with pytest.raises(RfqError):
        codec.set_option("RFQ_JUDGE", "fast")


# ---- 10: text -> judge -> select -> text
def test_text_judge_select_text(codec):
    J.check_composition(codec)


# ---- 11: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", J.W.WALK_IDS)
def test_walk_seams(codec, case):
    J.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    J.check_walk_bad_length(codec)
