"""CPU: rfq_decode_names - the name lines of an image and their offsets, in the layout rfq_rows_in takes - under the SIMT interpreter, against the
names of the plain-C oracle's text (tests/_names.py).  The GPU twin is tests/test_gpu_names.py."""
import pytest

import _engine as E
import _names as N
import _oracle as O
import _rows as W
import _rows_enc as R
from cases import CASES


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


def _oracle_rfq(case):
    try:
        return O.encode_file(case["fq1"], case.get("fq2", b""), case["paired"], case.get("k", 1000) * 1000)
    except O.OracleError:
        return None


DECODABLE = sorted(n for n in CASES if n != "se_name_over_255" and _oracle_rfq(CASES[n]) is not None)


# ---- 1: oracle parity on existing fixtures
@pytest.mark.parametrize("name", DECODABLE)
def test_case_names_like_oracle(codec, name):
    N.check(codec, _oracle_rfq(CASES[name]))


@pytest.mark.parametrize("label", [g[0] for g in W.GENERATED])
def test_generated_names_like_oracle(codec, label):
    assert len(N.check(codec, W.generated(label))) > 100


# ---- 2: small shapes where the writer can go wrong
def test_unparsed_names_at_every_residue_and_beyond_the_tile(codec):
    rfq, names = N.unparsed_names()
    assert N.check(codec, rfq) == names


def test_illumina_names_across_digit_counts(codec):
    rfq, names = N.illumina_digit_counts()
    assert N.check(codec, rfq) == names


def test_coordinates_of_eight_digits_and_more_are_not_storable():
    assert all(e and "cannot be larger than 2M" in e for e in N.coordinates_beyond_the_format())


@pytest.mark.parametrize("shape", [s[0] for s in N.pe_shapes()])
def test_pe_mates_and_name2(codec, shape):
    N.check(codec, dict(N.pe_shapes())[shape])


@pytest.mark.parametrize("shape", [s[0] for s in N.tiny_shapes()])
def test_tiny_shapes(codec, shape):
    N.check(codec, dict(N.tiny_shapes())[shape])


# ---- 3: ranges and walks
@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_ranges_forced_by_slice_bases(codec, walk):
    rfq = W.generated("pe150")
    codec.set_option("RFQ_SLICE_BASES", str(45000))                    # two or three chunks of 20 k bases per range
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    N.check(codec, rfq)
    assert {"walk", "name_lens", "names"} <= set(dict(codec.timings())), codec.timings()
    N.check_size_only(codec, rfq)                                      # (the first of the two passes over the ranges alone)


@pytest.mark.parametrize("walk", ["guess", "exact"])
def test_chunk_index(codec, walk):
    rfq = W.generated("bgi_q40")
    if walk == "exact":
        codec.set_option("RFQ_WALK", "exact")
    N.check(codec, rfq, chunk_off=O.chunk_table(rfq))


@pytest.mark.parametrize("step", [700, 5000])
def test_image_slices_concatenate_to_the_whole(codec, step):
    rfq = W.generated("pe150")
    assert N.decode_names_in_slices(codec, rfq, step) == N.expected(rfq)


# ---- 4: size query and refusals
def test_size_query_guarded_buffers_and_refusals(codec):
    N.check_sizes_and_refusals(codec)


def test_empty_image(codec):
    d = codec.dev_put(b"x")
    try:
        r = codec.decode_names(d, 0)
        assert (r.n_rows, r.names_len, r.n_chunks, r.max_name) == (0, 0, 0, 0)
        assert codec.dev_get(r.d_name_off, 8) == b"\0" * 8
    finally:
        codec.dev_free(d)


# ---- 5: the loop closes
def test_rows_and_device_names_reencode_to_the_oracle_image(codec):
    took = [label for label in R.LABELS if N.check_loop(codec, label)]
    assert len(took) >= 3 and {"pe150", "se_var"} <= set(took), took


# ---- 6: hostile images
HOSTILE_COUNTS = dict(flip=10, header=5, fixed=8, lengths=5, quality=5, index=12)


def test_hostile_images_tame_subset(codec):
    s = N.run_hostile(codec, counts=HOSTILE_COUNTS, good_every=8, tame=True, time_bound_s=30.0)
    assert s["mutants"] >= 150 and s["good_checks"] >= 20 and s["errors"].get("FORMAT", 0) > 20 and s["decoded"] > 20, s
