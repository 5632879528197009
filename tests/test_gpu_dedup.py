"""GPU (MI355X): rfq_dedup_rows and repaq_amd.tensors.dedup_rows on the product library - rows to a keep byte that leaves one unit of every class of identical
units, the representative and the size of every class, a histogram and a summary - against a Python dict from key bytes to members (tests/_dedup.py).  The CPU
twin is tests/test_emu_dedup.py; the contention test lives only here."""
import pytest

import _dedup as D
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


# ---- 1: planted classes
@pytest.mark.parametrize("pairs", [False, True], ids=["rows", "pairs"])
@pytest.mark.parametrize("row_len", D.ROW_LENS)
def test_planted_classes(codec, row_len, pairs):
    D.check_planted(codec, row_len, pairs)


# ---- 2: near misses
def test_one_byte_changed_at_every_position(codec):
    D.check_every_position(codec)


def test_lengths_padding_case_and_empty_rows(codec):
    D.check_lengths_and_padding(codec)


def test_key_len(codec):
    D.check_key_len(codec)


def test_pairs_are_keyed_mate_by_mate(codec):
    D.check_pairs(codec)


# ---- 3: best quality
def test_best_quality(codec):
    D.check_best_quality(codec)


# ---- 4: candidates
def test_candidates(codec):
    D.check_candidates(codec)


# ---- 5: shapes and outputs
def test_shapes_and_outputs(codec):
    D.check_shapes_and_outputs(codec)


# ---- 6: state
def test_nothing_is_left_of_an_earlier_table(codec):
    D.check_state(codec, make_codec)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    D.check_host_refusals(codec)


@pytest.mark.parametrize("label", D.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    D.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    D.check_option(codec, E.reset_options)


# ---- 8: text -> judge -> dedup -> select -> text
def test_text_judge_dedup_select_text(codec):
    D.check_composition(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_judge_dedup_select_with_tensors(codec, side_stream):
    """the same two texts through fastq_to_tensors -> judge_rows -> dedup_rows -> select_rows -> rows_to_fastq give the host's texts, and dedup_rows' tensors
    are the reference's"""
    import numpy as np
    import torch
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, judge_rows, dedup_rows, select_rows, rows_to_fastq
    t1, t2 = D.compose_text()
    w1, w2, kept, dups = D.compose_expected(t1, t2, J.COMPOSE)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    c = dict(J.COMPOSE); flags = c.pop("cut_flags")
    c.update(cut_front=bool(flags & J.FRONT), cut_right=bool(flags & J.RIGHT), cut_tail=bool(flags & J.TAIL))
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        j = judge_rows(codec, t, codes=False, **c)
        d = dedup_rows(codec, t, pairs=True, keep=j["keep"], hist_len=8)
        d2 = dedup_rows(codec, t, pairs=True, keep=j["keep"].bool(), best_qual=True, key_len=50)
        s = select_rows(codec, t, keep=d["keep"], start=j["start"], length=j["length"], pairs=True, min_len=c["min_len"])
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
    stream.synchronize()
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2 and int(s["lens"].numel()) == 2 * kept
    B, Q, lens, cand = (x.cpu().numpy() for x in (t["bases"], t["quals"], t["lens"], j["keep"]))
    for got, e in ((d, D.expected(B, Q, lens, pairs=True, cand=cand, hist_len=8)), (d2, D.expected(B, Q, lens, pairs=True, cand=cand, best=True, key_len=50))):
        for k in ("keep", "dup_of", "count") + (("hist",) if "hist" in got else ()):
            assert np.array_equal(got[k].cpu().numpy().astype(np.int64), e[k].astype(np.int64)), k
        assert got["summary"] == e["summary"]
    assert d["summary"]["n_classes"] == kept and d["summary"]["n_dups"] == dups
    assert d["keep"].dtype == torch.uint8 and d["dup_of"].dtype == torch.int32 and d["count"].dtype == torch.int32 and d["hist"].dtype == torch.int64 and "hist" not in d2


# ---- 9: contention
def test_hot_slots(codec):
    """2^17 units of 32 bytes, half of them in 64 classes of about a thousand members - every member of a class goes for ONE slot, from many workgroups at a
    time - and the other half unique.  The result has to BE the reference's, in both modes and both times: whichever member claims a slot, and in whatever order
    the others arrive, the class, its representative and its size are the same.  (A condition the tree meets every time, not a rate.)"""
    import numpy as np
    rng = np.random.default_rng(41)
    U, L, hot = 1 << 17, 32, 64
    keys = D.ALPHA[rng.integers(0, 4, (U // 2 + hot, L))]
    cls = np.concatenate([rng.integers(0, hot, U // 2), hot + np.arange(U // 2)])
    cls = cls[rng.permutation(U)]
    B = np.ascontiguousarray(keys[cls]); Q = rng.integers(0, 42, (U, L)).astype(np.uint8); lens = np.full(U, L, np.int32)
    dev = D.dev_rows(codec, B, Q, lens)
    try:
        for best in (False, True):
            e = D.expected(B, Q, lens, best=best, hist_len=1024)
            assert D.sizes_of(e)[-hot] > 900 and e["summary"]["n_classes"] == U // 2 + hot
            first = None
            for _ in range(2):
                out, summ, raw = D.run(codec, dev, best=best, hist_len=1024)
                D.compare(out, summ, e, "hot slots, best %d:" % best)
                assert first is None or first == raw
                first = raw
    finally:
        dev.free()


# ---- 12: the seams of the shared walk (unit counts around a wave, a step, a workgroup; row lengths around each kernel)
@pytest.mark.parametrize("case", [x for x in D.W.WALK_IDS if "general" not in x])
def test_walk_seams(codec, case):
    D.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    D.check_walk_bad_length(codec)
