"""GPU (MI355X, the product library): the loose slots' N bits, stored only where a base is N and zeroed again behind their readers (tests/_nbits.py) - the twin
of tests/test_emu_nbits.py."""
import pytest

import _engine as E
import _nbits as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make():
    import torch
    assert torch.cuda.is_available()
    from repaq_amd import RfqCodec
    made = []

    def make_codec():
        c = RfqCodec(device=0, library=E.PRODUCT_LIB)
        assert "gfx950" in c.version()
        E.reset_options(c)                      # (whatever the environment says)
        made.append(c)
        return c
    yield make_codec
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def codec(make):
    return make()


@pytest.mark.parametrize("name", list(N.cases()))
def test_image_is_the_oracles(codec, name):
    N.check(codec, N.cases()[name])


@pytest.mark.parametrize("name", list(N.cases()))
def test_image_is_the_oracles_on_a_fresh_context(make, name):
    N.check(make(), N.cases()[name])


def test_every_input_behind_every_other(make):
    N.check_history(make)
