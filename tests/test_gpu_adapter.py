"""GPU (MI355X): rfq_adapter_rows and repaq_amd.tensors.trim_adapters on the product library - rows to the length adapter removal leaves, the detector that cut,
the pairs' insert sizes, a summary and an insert-size histogram - against plain loops over the shifts and positions on the host (tests/_adapter.py).  The CPU
twin is tests/test_emu_adapter.py."""
import pytest

import _adapter as A
import _engine as E

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


# ---- 1: shapes
@pytest.mark.parametrize("row_len", A.ROW_LENS)
def test_shapes(codec, row_len):
    A.check_shapes(codec, row_len)


# ---- 2: every shift
@pytest.mark.parametrize("lengths", A.EVERY_SHIFT_IDS)
def test_every_shift(codec, lengths):
    A.check_every_shift(codec, lengths)


# ---- 3: thresholds at equality
def test_thresholds_at_equality(codec):
    A.check_thresholds(codec)


# ---- 4: the order of the shifts
def test_order_of_the_shifts(codec):
    A.check_order(codec)


# ---- 5: base classes
def test_base_classes(codec):
    A.check_classes(codec)


# ---- 6: the adapter at every position
@pytest.mark.parametrize("adapter_len", A.ADAPTER_LENS)
def test_adapter_at_every_position(codec, adapter_len):
    A.check_adapter_positions(codec, adapter_len)


# ---- 7: both detectors
def test_both_detectors(codec):
    A.check_both(codec)


# ---- 8: degenerate
def test_degenerate(codec):
    A.check_degenerate(codec)


# ---- 9: each output alone, none, twice the same, the histogram
def test_outputs_and_histogram(codec):
    A.check_outputs(codec)


# ---- 10: refusals
def test_refused_on_the_host(codec):
    A.check_host_refusals(codec)


@pytest.mark.parametrize("label", A.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    A.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    assert "RFQ_ADAPTER" in codec.option_names()
    codec.set_option("RFQ_ADAPTER", "general")
    assert codec.get_option("RFQ_ADAPTER") == "general"
    E.reset_options(codec)
    assert codec.get_option("RFQ_ADAPTER") == ""
    codec.set_option("RFQ_ADAPTER", "staged")
    from repaq_amd import RfqError
    with pytest.raises(RfqError):
        codec.set_option("RFQ_ADAPTER", "fast")


def test_stage_time_is_reported(codec):
    import numpy as np
    B, lens = A.random_pairs(4, 40, 1, codes=True)
    A.check(codec, B, lens, A.shape_criteria(40)[2][1], True, paths=(None,))
    assert [n for n, _ in codec.timings()] == ["adapter:rows"] and np.isfinite(codec.timings()[0][1])


# ---- 11: text -> adapter -> judge -> select -> text
def test_text_adapter_judge_select_text(codec):
    A.check_composition(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_trim_adapters_with_tensors(codec, side_stream):
    """the composition's two texts through fastq_to_tensors -> trim_adapters -> judge_rows on the shortened lengths -> select_rows -> rows_to_fastq give the
    host's texts, and trim_adapters' tensors are the reference's"""
    import numpy as np
    import torch
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, trim_adapters, judge_rows, select_rows, rows_to_fastq
    t1, t2 = A.compose_text()
    fq1, fq2 = b"".join(t1), b"".join(t2)
    ca = dict(A.COMPOSE_A, hist_len=301)
    cj = J.crit(cut_flags=J.TAIL, cut_window=4, cut_mean_q=20, min_len=80, min_mean_q=20)
    w1, w2, kept, e = A.compose_expected([x for pair in zip(t1, t2) for x in pair], ca, cj, 80)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(fq1), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(fq2), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        r = trim_adapters(codec, t, codes=False, **ca)
        j = judge_rows(codec, dict(t, lens=r["length"]), codes=False, cut_tail=True, cut_window=4, cut_mean_q=20, min_len=80, min_mean_q=20)
        s = select_rows(codec, t, keep=j["keep"], start=j["start"], length=j["length"], pairs=True, min_len=80)
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
        single = trim_adapters(codec, t, codes=False, adapter1=A.AD1)
    stream.synchronize()
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2 and int(s["lens"].numel()) == 2 * kept
    for k, w in (("length", "length"), ("how", "how"), ("insert", "insert"), ("diff", "diff"), ("insert_hist", "hist")):
        assert np.array_equal(r[k].cpu().numpy().astype(np.int64), e[w].astype(np.int64)), k
    assert r["summary"] == e["summary"] and r["length"].dtype == torch.int32 and r["how"].dtype == torch.uint8 and r["insert_hist"].dtype == torch.int64
    B, lens = (t[k].cpu().numpy() for k in ("bases", "lens"))
    e1 = A.expected(B, lens, A.crit(adapter1=A.AD1, adapter_min=4, adapter_mm_per=8), False)
    assert set(single) == {"length", "how", "summary"} and np.array_equal(single["length"].cpu().numpy(), e1["length"]) and single["summary"] == e1["summary"]


# ---- 12: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", A.W.WALK_IDS)
def test_walk_seams(codec, case):
    A.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    A.check_walk_bad_length(codec)
