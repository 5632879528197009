"""CPU: rfq_rows_to_text and rfq_encode_rows - fixed-stride base / quality rows back to FASTQ text and to .rfq images - under the SIMT interpreter.
The expected text is each input's own text, the expected image the plain-C oracle's (tests/_rows_enc.py).  The GPU twin is tests/test_gpu_rows_encode.py."""
import pytest

import _engine as E
import _rows_enc as R


@pytest.fixture(scope="module")
def codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.build_emu())
    yield c
    c.close()


def test_enough_plain_cases():
    assert R.N_PLAIN_CASES >= 50 and len(R.INPUTS) == R.N_PLAIN_CASES + 4


@pytest.mark.parametrize("label", R.LABELS)
def test_rows_to_text_equals_the_text(codec, label):
    assert R.check_text_variants(codec, label) >= 4


@pytest.mark.parametrize("label", R.LABELS)
def test_encode_rows_equals_the_oracle_image(codec, label):
    """rfq_encode_rows == the oracle's image; the rows of rfq_decode_rows re-encode to it wherever the image holds the text's reads"""
    assert R.check_image(codec, label) == (label not in R.LOSSY)


def test_records_at_every_residue_across_workgroups(codec):
    R.check_shape(codec, R.residue_set())


def test_one_read_of_70000_bases(codec):
    R.check_shape(codec, R.long_read(), chunk_bases=100000)


def test_no_rows(codec):
    R.check_no_rows(codec)


@pytest.mark.parametrize("label", ["pe150", "se_var", "d6_tiny_pe_interleaved_in"])
def test_size_query_and_caps_one_byte_short(codec, label):
    R.check_sizes_and_short_caps(codec, label)


@pytest.mark.parametrize("label", R.REFUSAL_IDS)
def test_refusal_then_a_good_call(codec, label):
    R.check_refusal(codec, label, through_encoder=False)


@pytest.mark.parametrize("label", ["negative_length", "length_zero", "name_of_no_bytes", "code_5_mid_line", "qual_above_line_end", "name_newline_mid"])
def test_refusal_through_the_encoder(codec, label):
    R.check_refusal(codec, label, through_encoder=True)


def test_argument_refusals(codec):
    R.check_argument_refusals(codec)


@pytest.mark.parametrize("label", ["se_var", "pe150"])
def test_two_row_batches_make_one_file(codec, label):
    R.check_two_batches(codec, label, cut=250 if label == "se_var" else 120)


def test_stage_names(codec):
    R.check_stage_names(codec)
