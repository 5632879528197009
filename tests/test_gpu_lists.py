"""GPU (MI355X): the position-list passes of the fused decode (k_dec_pos_sum2 on the 16-bytes-per-lane front, k_dec_pos_link2, k_dec_pos_off, k_dec_pos_list) on the product library, on the
hand-made streams of tests/_lists.py - every lane, step and segment edge, under every RFQ_POS_SEG.  The CPU twin is tests/test_emu_lists.py."""
import pytest

import _engine as E
import _lists as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_back_to_default(codec):
    yield
    E.reset_options(codec)


@pytest.mark.parametrize("name", L.NAMES)
def test_stream_decodes_under_every_segment_size(codec, name):
    L.check(codec, name)


def test_segment_sizes_the_switch_takes(codec):
    from repaq_amd import RfqError
    for v in L.SEGS:
        codec.set_option("RFQ_POS_SEG", v)
        assert codec.get_option("RFQ_POS_SEG") == v
    for v in ("512", "1000", "8192"):
        with pytest.raises(RfqError):
            codec.set_option("RFQ_POS_SEG", v)
