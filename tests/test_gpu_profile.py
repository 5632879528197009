"""GPU (MI355X): rfq_profile_rows and repaq_amd.tensors.profile_rows on the product library - rows under a keep byte and a window per row to the tables of a QC
report and a summary per mate - against a numpy reference written from the rules (tests/_profile.py).  The CPU twin is tests/test_emu_profile.py; the contention
tests and the tensor wrapper live only here."""
import numpy as np
import pytest

import _engine as E
import _profile as P

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


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1: every table and the summary
@pytest.mark.parametrize("codes", [False, True], ids=["ascii", "codes"])
@pytest.mark.parametrize("pairs", [False, True], ids=["rows", "pairs"])
@pytest.mark.parametrize("row_len", P.ROW_LENS)
def test_tables_and_summary(codec, row_len, pairs, codes):
    P.check_tables(codec, row_len, pairs, codes)


@pytest.mark.parametrize("case", P.W.WALK_IDS)
def test_walk_seams_and_step_counts(codec, case):
    P.check_walk(codec, case, n_cu())


# ---- 2: windows
def test_windows_cycles_and_bins(codec):
    P.check_windows(codec)


# ---- 3: masks
def test_masks(codec):
    P.check_masks(codec)


# ---- 4: outputs
def test_each_output_alone_all_and_none(codec):
    P.check_outputs(codec)


# ---- 5: state
def test_nothing_is_left_of_an_earlier_call(codec):
    P.check_state(codec, make_codec, P.other_calls)


# ---- 6: agreement inside the family
def test_agrees_with_judge_and_select(codec):
    P.check_family(codec)


# ---- 7: contention
def _twice_on_both_paths(codec, B, Q, lens, e, kw):
    dev = P.dev_rows(codec, B, Q, lens)
    try:
        first = None
        for path in P.PATHS:
            codec.set_option(P.OPTION, path)
            for _ in range(2):
                out, summ, raw = P.run(codec, dev, False, **kw)
                P.compare(out, summ, e, "contention, path %s:" % (path or "default"))
                assert first is None or first == raw, "the raw bytes differ between runs or paths"
                first = raw
    finally:
        codec.set_option(P.OPTION, None)
        dev.free()


def test_every_lane_on_the_same_cells(codec):
    """2^16 rows of the same 32 bytes at one score: every group of every workgroup goes for the same cells at the same time.  The tables have to BE the reference's -
    the tables of one such row, times the rows: a table is a sum over rows - on both paths and both times, and the raw bytes equal.  (A condition the tree meets every
    time, not a rate.)"""
    n, L = 1 << 16, 32
    B = np.tile(np.frombuffer(b"ACGTNGGCATTACGNNacgtGCGCGCGCATAT", np.uint8), (n, 1)); Q = np.full((n, L), 37, np.uint8); lens = np.full(n, L, np.int32)
    kw = dict(pairs=True, cycles=L, qbins=42, len_bins=L + 1)
    one = P.expected(B[:2], Q[:2], lens[:2], False, **kw)
    e = {k: one[k] * np.uint64(n // 2) for k in P.TABLES}
    e["summary"] = dict({f: [v * (n // 2) for v in one["summary"][f]] for f in P.FIELDS}, n_rows=n, max_len=L)
    assert int(e["qual_hist"][0, 5, 37]) == n // 2 and int(e["len_hist"][1, L]) == n // 2
    _twice_on_both_paths(codec, B, Q, lens, e, kw)


def test_random_rows_under_contention(codec):
    n, L = 1 << 16, 32
    B, Q, lens = P.random_rows(n, L, 77, False, lo=20)
    kw = dict(pairs=True, cycles=L, qbins=42, len_bins=L + 1)
    _twice_on_both_paths(codec, B, Q, lens, P.expected(B, Q, lens, False, **kw), kw)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    P.check_host_refusals(codec)


@pytest.mark.parametrize("label", P.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    P.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    P.check_option(codec, E.reset_options)


# ---- 9: the tensor wrapper
@pytest.mark.parametrize("side_stream", [False, True])
def test_profile_rows_with_tensors(codec, side_stream):
    """fastq_to_tensors -> judge_rows -> profile_rows before and under the judge's triple, bool and uint8 keep: the reference's tables, int64, shaped as documented"""
    import torch
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, judge_rows, profile_rows
    t1, t2 = J.compose_text(pairs=200)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    c = dict(J.COMPOSE); flags = c.pop("cut_flags")
    c.update(cut_front=bool(flags & J.FRONT), cut_right=bool(flags & J.RIGHT), cut_tail=bool(flags & J.TAIL))
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        j = judge_rows(codec, t, codes=False, **c)
        before = profile_rows(codec, t, pairs=True, codes=False)
        after = profile_rows(codec, t, pairs=True, codes=False, keep=j["keep"], start=j["start"], length=j["length"], qbins=42)
        after_b = profile_rows(codec, t, pairs=True, codes=False, keep=j["keep"].bool(), start=j["start"], length=j["length"], qbins=42, cycles=50, len_bins=8,
                               tables=("qual_hist", "len_hist"))
        single = profile_rows(codec, t, codes=False, length=j["length"])
    stream.synchronize()
    B, Q, lens, keep, start, length = (x.cpu().numpy() for x in (t["bases"], t["quals"], t["lens"], j["keep"], j["start"], j["length"]))
    L = B.shape[1]
    for got, M, e in ((before, 2, P.expected(B, Q, lens, False, True, None, None, None, L, 64, L + 1)),
                      (after, 2, P.expected(B, Q, lens, False, True, keep, start, length, L, 42, L + 1)),
                      (after_b, 2, P.expected(B, Q, lens, False, True, keep, start, length, 50, 42, 8)),
                      (single, 1, P.expected(B, Q, lens, False, False, None, None, length, L, 64, L + 1))):
        tables = [k for k in got if k != "summary"]
        assert set(tables) == (set(P.TABLES) if got is not after_b else {"qual_hist", "len_hist"})
        for k in tables:
            assert got[k].dtype == torch.int64 and tuple(got[k].shape) == e[k].shape and got[k].device == dev, k
            assert np.array_equal(got[k].cpu().numpy().astype(np.uint64), e[k]), k
        assert got["summary"] == e["summary"] and len(got["summary"]["bases"]) == M
    assert sum(after["summary"]["bases"]) == j["summary"]["bases_out"] and sum(before["summary"]["q30"]) == j["summary"]["q30_in"]
