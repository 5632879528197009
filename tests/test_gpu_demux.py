"""GPU (MI355X): rfq_demux_rows and repaq_amd.tensors.demux_rows / split_rows on the product library - rows against one or two sets of barcodes to a sample per unit,
the reason where there is none, the keep byte and start rfq_select_rows takes and a count per sample - against a plain Python loop over units, barcodes and positions
(tests/_demux.py).  The CPU twin is tests/test_emu_demux.py; the composition with the tensors lives only here."""
import pytest

import _demux as D
import _engine as E


pytestmark = pytest.mark.gpu


def make_codec():
    from repaq_amd import RfqCodec
    c = RfqCodec(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    return c


@pytest.fixture(scope="module")
def codec():
    c = make_codec()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _options_back_to_default(codec):
    yield
    E.reset_options(codec)


# ---- 1: every barcode at every distance (6: on both formulations, equal bytes)
@pytest.mark.parametrize("ln", D.PLANT_LENS)
def test_every_barcode_exact_one_mismatch_n_and_lower_case(codec, ln):
    D.check_every_distance(codec, ln)


# ---- 2: window seams
@pytest.mark.parametrize("off", D.SEAM_OFFS)
def test_windows_across_group_row_and_buffer_seams(codec, off):
    D.check_seams(codec, off)


# ---- 3: ties and deltas
def test_ties_deltas_one_barcode_and_4096(codec):
    D.check_ties(codec)


# ---- 4: pairs
def test_pairs_two_sets_sheet_every_reason_alone_masked_mates(codec):
    D.check_pairs(codec)


# ---- 5: the walk
@pytest.mark.parametrize("case", D.WALK_IDS)
def test_walk_seams(codec, case):
    D.check_walk(codec, case)


def test_walk_bad_length_in_the_last_row(codec):
    D.check_walk_bad_length(codec)


@pytest.mark.parametrize("cells", (8192, 8193))
def test_counts_in_lds_and_in_device_memory(codec, cells):
    D.check_counts_paths(codec, cells)


def test_the_largest_sets_and_count_table_the_lds_holds(codec):
    D.check_lds_max(codec)


# ---- 6: the switch
def test_the_switch_is_listed_and_resets(codec):
    D.check_option(codec, E.reset_options)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    D.check_host_refusals(codec)


@pytest.mark.parametrize("label", D.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    D.check_device_refusal(codec, label)


# ---- 8: state
def test_a_demux_leaves_other_calls_alone_and_sets_of_any_size_follow_each_other(codec):
    D.check_state(codec)


# ---- 5: more units than a step of the capped grid
def test_many_short_rows_take_several_steps(codec):
    D.check_many_rows(codec)


# ---- 9: composition with tensors
@pytest.mark.parametrize("side_stream", [False, True])
def test_fastq_demux_split_fastq_with_tensors(codec, side_stream):
    """two paired texts with inline barcodes through fastq_to_tensors -> demux_rows -> split_rows(start=...) -> rows_to_fastq give, per sample and for the unassigned
    bin, the host model's texts byte for byte; demux_rows' tensors are the model's, with the dtypes the docstrings name"""
    import numpy as np
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, demux_rows, split_rows, rows_to_fastq
    (t1, t2), set1, set2, sheet = D.compose_text()
    want, e = D.compose_expected(t1, t2, set1, set2, sheet)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        dm = demux_rows(codec, t, [x.decode() for x in set1], set2, sheet=sheet, pairs=True, codes=False, **D.COMPOSE)
        parts = split_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True)
        got = [rows_to_fastq(codec, p["bases"], p["quals"], p["lens"], p["names"], p["name_off"], paired=PE_TWO_FILES, codes=False) if p is not None else None for p in parts]
    stream.synchronize()
    assert len(parts) == len(sheet) + 1
    # the pairs with a read that its barcode used up are in no bin, and the bins say so
    assert e["dropped"] >= 1 and sum(int(p["lens"].numel()) for p in parts if p is not None) == 2 * (len(t1) - e["dropped"])
    assert sum(p["dropped"]["short"] + p["dropped"]["mate"] for p in parts if p is not None) == 2 * e["dropped"]
    for k, (w1, w2) in enumerate(want):
        if got[k] is None:
            assert w1 == b"" and w2 == b"", k
        else:
            assert bytes(got[k][0].cpu().numpy().tobytes()) == w1 and bytes(got[k][1].cpu().numpy().tobytes()) == w2, "the texts of bin %d differ" % k
    for k in ("sample", "why", "best", "dist", "keep", "start", "counts"):
        assert np.array_equal(dm[k].cpu().numpy().astype(np.int64), e[k].astype(np.int64)), k
    assert dm["summary"] == e["summary"]
    s = e["summary"]
    assert s["why_combo"] > 0 and s["why_none"] > 0 and s["why_short"] > 0 and s["n_exact"] < s["n_assigned"] and all(w1 for w1, _ in want)
    assert dm["sample"].dtype == torch.int32 and dm["why"].dtype == torch.uint8 and dm["best"].dtype == torch.int32 and dm["dist"].dtype == torch.uint8
    assert dm["keep"].dtype == torch.uint8 and dm["start"].dtype == torch.int32 and dm["counts"].dtype == torch.int64
    # a keep mask from an earlier step, as bool
    keep = torch.ones(dm["keep"].numel(), dtype=torch.bool, device=dev); keep[5] = False
    dm2 = demux_rows(codec, t, set1, set2, sheet=sheet, pairs=True, codes=False, keep=keep, **D.COMPOSE)
    assert int(dm2["why"][2]) == D.MASKED and dm2["summary"]["n_candidates"] == s["n_candidates"] - 1
