"""CPU: rfq_profile_rows - rows under a keep byte and a window per row to the tables of a QC report (base content and score sum per cycle, position x score, the
distributions of length, mean score and GC content) and a summary per mate - under the SIMT interpreter, against a numpy reference written from the rules
(tests/_profile.py).  The GPU twin is tests/test_gpu_profile.py (it adds the contention tests - the interpreter runs a workgroup's lanes one after the other and
cannot show a race - and the tensor wrapper); tools/profile_asan.sh runs the good shapes and the refusals through a stand-alone AddressSanitizer + UBSan program
of the same sources."""
import pytest

import _engine as E
import _profile as P


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


# ---- 1: every table and the summary
@pytest.mark.parametrize("codes", [False, True], ids=["ascii", "codes"])
@pytest.mark.parametrize("pairs", [False, True], ids=["rows", "pairs"])
@pytest.mark.parametrize("row_len", P.ROW_LENS)
def test_tables_and_summary(codec, row_len, pairs, codes):
    P.check_tables(codec, row_len, pairs, codes)


@pytest.mark.parametrize("case", P.W.WALK_IDS)
def test_walk_seams_and_step_counts(codec, case):
    P.check_walk(codec, case, P.EMU_CUS)


# ---- 2: windows
def test_windows_cycles_and_bins(codec):
    P.check_windows(codec)


# ---- 3: masks
def test_masks(codec):
    P.check_masks(codec)


# ---- 4: outputs
def test_each_output_alone_all_and_none(codec):
    P.check_outputs(codec)


# ---- 5: state
def test_nothing_is_left_of_an_earlier_call(codec):
    P.check_state(codec, make_codec, P.other_calls)


# ---- 6: agreement inside the family
def test_agrees_with_judge_and_select(codec):
    P.check_family(codec)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    P.check_host_refusals(codec)


@pytest.mark.parametrize("label", P.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    P.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    P.check_option(codec, E.reset_options)
