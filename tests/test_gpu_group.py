"""GPU (MI355X): rfq_group_rows and repaq_amd.tensors.group_rows / group_parts on the product library - rfq_select_rows with the kept rows grouped by a bin per
unit in one pass - against a numpy / Python model and, bin by bin, against rfq_select_rows of the same library under the bin's mask (tests/_group.py).  The sort
works in tiles of GR_TILE = 2048 elements.  The CPU twin is tests/test_emu_group.py; the composition with the tensors lives only here."""
import pytest

import _engine as E
import _group as G


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


# ---- 1: unit counts
@pytest.mark.parametrize("units", G.UNITS)
def test_unit_counts_around_a_wave_a_step_and_a_tile(codec, units):
    G.check_units(codec, units)


def test_many_units_take_many_workgroups(codec):
    G.check_many_units(codec)


# ---- 2: total bins
@pytest.mark.parametrize("total", G.TOTALS)
def test_total_bins_one_pass_two_passes_and_the_limits(codec, total):
    G.check_totals(codec, total)


# ---- 3: bin patterns
@pytest.mark.parametrize("pattern", G.PATTERN_IDS)
def test_bin_patterns(codec, pattern):
    G.check_pattern(codec, pattern)


# ---- 4: the rest bin
def test_rest_bin_or_dropped_with_and_without_negative_bins(codec):
    G.check_rest(codec)


# ---- 5: pairs
def test_pairs_stay_adjacent_and_fall_with_their_mate(codec):
    G.check_pairs(codec)


# ---- 6: names
def test_rows_without_names_empty_names_and_a_long_name(codec):
    G.check_names(codec)


# ---- 7: layout, no rows left, partial outputs, determinism
def test_unaligned_and_aligned_row_buffers(codec):
    G.check_layout(codec)


def test_nothing_kept_writes_one_offset_and_zero_bin_offsets(codec):
    G.check_nothing_kept(codec)


def test_partial_outputs_and_bin_offsets_alone(codec):
    G.check_partial_outputs(codec)


def test_the_same_call_twice_writes_the_same_bytes(codec):
    G.check_same_bytes_twice(codec)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    G.check_host_refusals(codec)


def test_short_caps_are_nospace_and_nothing_is_written(codec):
    G.check_short_caps(codec)


@pytest.mark.parametrize("label", G.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    G.check_device_refusal(codec, label)


def test_a_bad_bin_beside_selects_device_refusals(codec):
    G.check_device_refusals_together(codec)


# ---- 9: state
def test_scratch_at_other_sizes_other_calls_unchanged_good_after_refused(codec):
    G.check_state(codec)


# ---- 10: composition with tensors
@pytest.mark.parametrize("side_stream", [False, True])
def test_fastq_demux_group_parts_fastq_with_tensors(codec, side_stream):
    """two paired texts with inline barcodes through fastq_to_tensors -> demux_rows -> group_rows(bin=sample, start=...) -> group_parts -> rows_to_fastq give, per
    sample and for the rest bin, the host model's texts byte for byte, and part for part what split_rows returns for the same inputs"""
    import numpy as np
    import torch
    import _demux as D
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, demux_rows, split_rows, group_rows, group_parts, rows_to_fastq
    (t1, t2), set1, set2, sheet = D.compose_text()
    want, e = D.compose_expected(t1, t2, set1, set2, sheet)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        dm = demux_rows(codec, t, [x.decode() for x in set1], set2, sheet=sheet, pairs=True, codes=False, **D.COMPOSE)
        g = group_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True)
        parts = group_parts(g)
        got = [rows_to_fastq(codec, p["bases"], p["quals"], p["lens"], p["names"], p["name_off"], paired=PE_TWO_FILES, codes=False) if p is not None else None for p in parts]
        split = split_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True)
    stream.synchronize()
    T = len(sheet) + 1
    assert len(parts) == T == len(split)
    assert g["bin_off"].dtype == torch.int64 and g["bin_off"].device == t["bases"].device and g["bin_off"].numel() == T + 1
    assert int(g["bin_off"][T]) == int(g["lens"].numel()) == 2 * (len(t1) - e["dropped"]) and e["dropped"] >= 1
    assert g["dropped"] == {"mask": 0, "bin": 0, "short": g["dropped"]["short"], "mate": g["dropped"]["mate"]} and g["dropped"]["short"] + g["dropped"]["mate"] == 2 * e["dropped"]
    for k, (w1, w2) in enumerate(want):
        if got[k] is None:
            assert w1 == b"" and w2 == b"" and split[k] is None, k
            continue
        assert bytes(got[k][0].cpu().numpy().tobytes()) == w1 and bytes(got[k][1].cpu().numpy().tobytes()) == w2, "the texts of bin %d differ" % k
        p, s = parts[k], split[k]
        assert p["bases"].dtype == torch.uint8 and p["quals"].dtype == torch.uint8 and p["lens"].dtype == torch.int32 and p["names"].dtype == torch.uint8
        assert p["name_off"].dtype == torch.int64 and all(v.device == t["bases"].device and v.is_contiguous() for v in p.values())
        assert torch.equal(p["lens"], s["lens"]) and torch.equal(p["names"], s["names"]) and torch.equal(p["name_off"], s["name_off"]), "bin %d differs from split_rows'" % k
        lp, ls = p["bases"].shape[1], s["bases"].shape[1]                     # (split_rows pads every bin to its own longest row)
        inside = (torch.arange(lp, device=dev)[None, :] < p["lens"][:, None])
        for key in ("bases", "quals"):
            x = torch.where(inside, p[key], torch.zeros_like(p[key]))[:, :ls]
            y = torch.where(inside[:, :ls], s[key], torch.zeros_like(s[key]))
            assert ls <= lp and torch.equal(x, y) and not bool(inside[:, ls:].any()), "bin %d: the %s up to each length differ from split_rows'" % (k, key)
    assert all(w1 for w1, _ in want)
    # rest=False drops the unassigned pairs and says so
    with torch.cuda.stream(stream):
        g2 = group_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True, rest=False)
    stream.synchronize()
    none = int((dm["sample"] < 0).sum())
    assert g2["bin_off"].numel() == T and g2["dropped"]["bin"] == 2 * none and torch.equal(g2["bin_off"], g["bin_off"][:T])
