"""CPU: rfq_text_rows - FASTQ text to per-read base / quality rows, lengths and names - under the SIMT interpreter, against the text's own lines
(plain texts) or the plain-C oracle's round trip (the reader's quirks): tests/_text_rows.py.  The GPU twin is tests/test_gpu_text_rows.py; tools/text_rows_asan.sh
runs the good inputs and the junk of test 8 through a stand-alone AddressSanitizer + UBSan program of the same sources (log: profiles/r10_text_rows_asan.txt)."""
import pytest

import _engine as E
import _rows_enc as R
import _text_rows as T


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


# ---- 1: every golden case
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_case_rows_and_names(codec, name):
    assert T.check_case(codec, name) == T.ROUTES[name]


# ---- 2: generated inputs over the row variants, text at shifts 1 / 7 / 15
@pytest.mark.parametrize("label", T.GEN_LABELS)
def test_generated_over_variants(codec, label):
    T.check_generated(codec, label)


# ---- 3: small shapes
def test_read_lengths_and_names_at_every_residue(codec):
    T.check_shapes(codec)


def test_one_record_with_and_without_final_newline(codec):
    T.check_one_record_and_final(codec)


def test_long_read_and_pad_fill(codec):
    T.check_long_read_and_pad(codec)


def test_each_output_alone(codec):
    T.check_each_output_alone(codec)


# ---- 4: pairs
def test_pairs_two_files_and_interleaved(codec):
    T.check_pairs(codec)


# ---- 5: streaming
@pytest.mark.parametrize("step", [997, 20011])
def test_text_fed_in_steps_equals_one_shot(codec, step):
    T.check_streaming(codec, step)


def test_forced_slices_consume_less_and_the_loop_equals_one_shot(codec):
    T.check_streaming_forced_slices(codec)


# ---- 6: sizes and refusals
def test_caps_one_short(codec):
    T.check_short_caps(codec)


def test_quality_line_one_short_and_one_long(codec):
    T.check_quality_lengths(codec)


def test_argument_refusals(codec):
    T.check_argument_refusals(codec)


def test_empty_text(codec):
    T.check_empty_text(codec)


# ---- 7: closing the square
@pytest.mark.parametrize("label", R.LABELS)
def test_text_rows_back_to_text_and_to_the_oracle_image(codec, label):
    T.check_square(codec, label)


# ---- 8: junk that is still input
def test_junk_returns_rows_or_a_code(codec):
    s = T.run_junk(codec)
    assert s["calls"] == 72 and s["rows"] > 0 and s["errors"], s
