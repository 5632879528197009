"""CPU: rfq_merge_rows - every pair with an insert size to one row, the consensus of both mates, under R1's name - under the SIMT interpreter, against plain loops
over the fragment's positions on the host (tests/_merge.py).  The GPU twin is tests/test_gpu_merge.py; tools/merge_asan.sh runs the shapes, every insert and the
refusals through a stand-alone AddressSanitizer + UBSan program of the same sources (log: profiles/r18_merge_asan.txt)."""
import pytest

import _engine as E
import _merge as M


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
@pytest.mark.parametrize("row_len", M.ROW_LENS)
def test_shapes(codec, row_len):
    M.check_shapes(codec, row_len)


# ---- 2: every insert
@pytest.mark.parametrize("lengths", M.EVERY_INSERT_IDS)
def test_every_insert(codec, lengths):
    M.check_every_insert(codec, lengths)


def test_every_insert_reaches_both_ends_of_the_buffer():
    M.check_load_edges_are_reached()


# ---- 3: the consensus table
@pytest.mark.parametrize("codes", [True, False], ids=["codes", "ascii"])
def test_consensus_table(codec, codes):
    M.check_consensus_table(codec, codes)


# ---- 4: an oracle that does not share the rule's code
def test_fragments_come_back(codec):
    M.check_fragments(codec)


# ---- 5: nothing, everything, degenerate
def test_degenerate(codec):
    M.check_degenerate(codec)


# ---- 6: names
def test_names(codec):
    M.check_names(codec)


# ---- 7: outputs
def test_outputs_and_caps(codec):
    M.check_outputs(codec)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    M.check_host_refusals(codec)


@pytest.mark.parametrize("label", M.DEVICE_REFUSALS)
def test_refused_on_the_device(codec, label):
    M.check_device_refusal(codec, label)


# ---- 9: the switch and the timings
def test_the_switch_and_the_stage_times(codec):
    M.check_switch_and_timings(codec)


# ---- 10: text -> adapter -> merge -> text
def test_text_adapter_merge_text(codec):
    M.check_composition(codec)
