"""CPU: rfq_select_rows - rows to the kept rows, trimmed to a window each, with their lengths, names and name offsets - under the SIMT interpreter, against
numpy on the host (tests/_select.py).  The GPU twin is tests/test_gpu_select.py; tools/select_asan.sh runs the good shapes and the refusals through a stand-alone
AddressSanitizer + UBSan program of the same sources (log: profiles/r12_select_asan.txt)."""
import pytest

import _engine as E
import _rows_enc as R
import _select as S


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


# ---- 1: identity
@pytest.mark.parametrize("label", [g[0] for g in S.W.GENERATED])
def test_everything_kept_is_the_input(codec, label):
    S.check_identity(codec, label)


# ---- 2: windows at every residue, buffers at shifts 0 / 1 / 7 / 15
@pytest.mark.parametrize("row_len_in", S.WINDOW_ROW_LENS)
def test_windows_at_every_residue(codec, row_len_in):
    S.check_windows(codec, row_len_in)


# ---- 3: masks
@pytest.mark.parametrize("n_rows", S.MASK_ROWS)
def test_mask_patterns(codec, n_rows):
    S.check_masks(codec, n_rows)


# ---- 4: both forms of the scan
@pytest.mark.parametrize("n_rows", [16385])
def test_scan_small_and_tiled(codec, n_rows):
    S.check_scan(codec, n_rows)


# ---- 5: pairs and min_len
def test_pairs_and_min_len(codec):
    S.check_pairs_and_min_len(codec)


# ---- 6: names
def test_names_at_every_residue(codec):
    S.check_name_residues(codec)


def test_name_longer_than_a_tile(codec):
    S.check_long_name(codec)


def test_rows_without_names_and_each_output_alone(codec):
    S.check_no_names_and_each_output_alone(codec)


# ---- 7: sizes and refusals
def test_caps_one_short(codec):
    S.check_short_caps(codec)


@pytest.mark.parametrize("label", S.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    S.check_device_refusal(codec, label)


def test_refused_on_the_host(codec):
    S.check_host_refusals(codec)


# ---- 8: closing the square
@pytest.mark.parametrize("label", R.LABELS)
def test_text_rows_select_back_to_text_and_to_the_oracle_image(codec, label):
    S.check_square(codec, label)


# ---- 9: twice is the same
@pytest.mark.parametrize("label", [g[0] for g in S.W.GENERATED])
def test_twice_is_the_same(codec, label):
    S.check_square(codec, label, twice=True)
