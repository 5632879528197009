"""GPU (MI355X): rfq_judge_rows and repaq_amd.tensors.judge_rows / filter_rows on the product library - rows to a keep byte, a window, a reason byte and four
metrics per row and one QC summary - against a plain per-row loop on the host (tests/_judge.py).  The CPU twin is tests/test_emu_judge.py."""
import pytest

import _engine as E
import _judge as J

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


# ---- 1: every step alone, then all together
@pytest.mark.parametrize("row_len", J.ROW_LENS)
def test_every_step_alone_and_all_together(codec, row_len):
    J.check_steps(codec, row_len)


# ---- 2: window seams
@pytest.mark.parametrize("cut_window", [1, 4, 300, 500])
@pytest.mark.parametrize("kind", ["front", "right", "tail"])
def test_window_at_every_position(codec, kind, cut_window):
    J.check_seams(codec, kind, cut_window, trim=0 if cut_window != 4 else 2)


@pytest.mark.parametrize("kind", ["front", "right", "tail"])
def test_window_of_1000_on_a_longer_row(codec, kind):
    J.check_seams(codec, kind, 1000, L=1500, step=41)


# ---- 3: poly-G
def test_poly_g(codec):
    J.check_poly_g(codec)


# ---- 4: every reason at equality
def test_every_reason_at_equality(codec):
    J.check_reasons(codec)


# ---- 5: empty and degenerate
def test_empty_and_degenerate(codec):
    J.check_degenerate(codec)


# ---- 6: a long row, naturally
def test_long_rows(codec):
    J.check_long_rows(codec)


# ---- 7 and 8: each output alone, none, the summary, twice the same
def test_outputs_and_summary(codec):
    J.check_outputs_and_summary(codec)


# ---- 9: refusals
def test_refused_on_the_host(codec):
    J.check_host_refusals(codec)


@pytest.mark.parametrize("label", J.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    J.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    assert "RFQ_JUDGE" in codec.option_names()
    codec.set_option("RFQ_JUDGE", "general")
    E.reset_options(codec)
    assert codec.get_option("RFQ_JUDGE") == ""
    from repaq_amd import RfqError
    with pytest.raises(RfqError):
        codec.set_option("RFQ_JUDGE", "fast")


# ---- 10: text -> judge -> select -> text
def test_text_judge_select_text(codec):
    J.check_composition(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_filter_rows_with_tensors(codec, side_stream):
    """the same two texts through fastq_to_tensors -> filter_rows -> rows_to_fastq give the host's texts, encode_tensors -> decode_tensors of the filtered
    rows gives them back, and judge_rows' tensors are the reference's"""
    import numpy as np
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, filter_rows, judge_rows, rows_to_fastq, encode_tensors, decode_tensors
    t1, t2 = J.compose_text()
    fq1, fq2 = b"".join(t1), b"".join(t2)
    w1, w2, kept = J.compose_expected([x for pair in zip(t1, t2) for x in pair], J.COMPOSE, J.COMPOSE["min_len"])
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(fq1), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(fq2), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    c = dict(J.COMPOSE); flags = c.pop("cut_flags")
    c.update(cut_front=bool(flags & J.FRONT), cut_right=bool(flags & J.RIGHT), cut_tail=bool(flags & J.TAIL))
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        j = judge_rows(codec, t, codes=False, metrics=True, **c)
        s = filter_rows(codec, t, pairs=True, codes=False, **c)
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
        codec.clearHeader()
        img = encode_tensors(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False, chunk_bases=20000)
        d = decode_tensors(codec, img, codes=False, names=True)
    stream.synchronize()
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2 and int(s["lens"].numel()) == 2 * kept
    B, Q, lens = (t[k].cpu().numpy() for k in ("bases", "quals", "lens"))
    e = J.expected(B, Q, lens, J.COMPOSE, False)
    for k, w in (("keep", "keep"), ("start", "start"), ("length", "length"), ("why", "why"), ("metrics", "metrics")):
        assert np.array_equal(j[k].cpu().numpy().astype(np.int64), e[w].astype(np.int64)), k
    assert j["summary"] == e["summary"] == s["summary"] and j["keep"].dtype == torch.uint8 and j["start"].dtype == torch.int32
    L = int(s["lens"].max())
    assert torch.equal(d["lens"], s["lens"]) and torch.equal(d["names"], s["names"])
    inside = torch.arange(L, device=dev)[None, :] < s["lens"][:, None]
    assert torch.equal(d["bases"][:, :L][inside], s["bases"][:, :L][inside]) and torch.equal(d["quals"][:, :L][inside], s["quals"][:, :L][inside])


# ---- 11: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", J.W.WALK_IDS)
def test_walk_seams(codec, case):
    J.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    J.check_walk_bad_length(codec)
