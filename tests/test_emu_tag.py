"""CPU: rfq_select_rows with a tag (rfq_name_tag) - a tag of the read's own bases written into the kept names, UMI extraction - under the SIMT interpreter, against a
plain Python loop over rows that builds every expected name (tests/_tag.py).  The GPU twin is tests/test_gpu_tag.py (it adds the composition with the tensors);
tools/tag_asan.sh runs good shapes and the refusals through a stand-alone AddressSanitizer + UBSan program of the same sources."""
import pytest

import _engine as E
import _tag as G


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


# ---- 1: the place
@pytest.mark.parametrize("at", (G.AT_SPACE, G.AT_END), ids=("space", "end"))
def test_the_tag_goes_in_front_of_the_first_space_or_to_the_end(codec, at):
    G.check_place(codec, at)


# ---- 2: the seams of the blob
@pytest.mark.parametrize("out_shift", range(16))
def test_tags_across_group_and_tile_boundaries_at_every_alignment(codec, out_shift):
    G.check_blob_seams(codec, out_shift)


def test_more_than_256_names_start_in_a_tile_some_empty_and_untagged(codec):
    G.check_many_names_in_a_tile(codec)


# ---- 3: the parts
@pytest.mark.parametrize("codes", (False, True), ids=("ascii", "codes"))
def test_parts_of_every_length_at_every_start_and_at_the_end_of_the_buffer(codec, codes):
    G.check_parts(codec, codes)


# ---- 4: pairs
def test_pairs_share_one_tag_and_dropped_pairs_give_no_name(codec):
    G.check_pairs(codec)


# ---- 5: identity
def test_a_tag_of_empty_parts_is_the_plain_call(codec):
    G.check_identity(codec)


# ---- 6: sizes
def test_size_query_short_cap_and_no_rows(codec):
    G.check_sizes(codec)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    G.check_host_refusals(codec)


@pytest.mark.parametrize("label", G.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    G.check_device_refusal(codec, label)


# ---- 8: state
def test_tagged_plain_and_smaller_tagged_calls_follow_each_other(codec):
    G.check_state(codec)


def test_the_stages_of_a_tagged_call(codec):
    G.check_stage_names(codec)


# ---- 9: the switch
def test_the_switch_is_listed_and_resets(codec):
    G.check_option(codec, E.reset_options)
