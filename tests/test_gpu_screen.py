"""GPU (MI355X): rfq_screen_build, rfq_screen_rows and repaq_amd.tensors.screen_index / screen_rows on the product library - reference sequences to an exact set of
canonical k-mers, rows to their k-mers, their hits and a keep byte - against a Python set of canonical ints and a plain loop over the positions
(tests/_screen.py).  The CPU twin is tests/test_emu_screen.py; the contention test of the build and the tensors live only here."""
import pytest

import _engine as E
import _screen as S

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


# ---- 1: every position, every k
@pytest.mark.parametrize("k", S.KS)
def test_a_reference_kmer_at_every_position(codec, k):
    S.check_every_position(codec, k)


# ---- 2: validity
def test_other_bytes_short_rows_padding_and_a_palindrome(codec):
    S.check_validity(codec)


# ---- 3: seams
@pytest.mark.parametrize("row_len", S.SEAM_IDS)
def test_hits_across_lane_kernel_and_tile_seams(codec, row_len):
    S.check_seams(codec, row_len)


@pytest.mark.parametrize("case", S.W.WALK_IDS)
def test_walk_seams(codec, case):
    S.check_walk(codec, case)


def test_walk_bad_length_in_the_last_unit(codec):
    S.check_walk_bad_length(codec)


# ---- 4: the verdict
def test_verdict_boundaries_modes_pairs_candidates_outputs(codec):
    S.check_verdict(codec)


# ---- 5: the set
def test_the_set_of_a_reference_list(codec):
    S.check_set(codec)


def test_lds_and_device_memory_placement_agree(codec):
    S.check_placements(codec)


# ---- 6: refusals
def test_build_refused(codec):
    S.check_build_refusals(codec)


def test_rows_refused_on_the_host(codec):
    S.check_host_refusals(codec)


def test_an_index_that_is_none_and_an_index_that_is_full(codec):
    S.check_bad_index(codec)


@pytest.mark.parametrize("label", S.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    S.check_device_refusal(codec, label)


def test_the_switch_is_listed_and_resets(codec):
    S.check_option(codec, E.reset_options)


# ---- 7: state and composition
def test_a_screen_leaves_other_calls_alone(codec):
    S.check_state(codec)


def test_text_adapter_judge_screen_dedup_select_text(codec):
    S.check_composition(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_adapter_judge_screen_dedup_select_with_tensors(codec, side_stream):
    """the same two texts through fastq_to_tensors -> trim_adapters -> judge_rows -> screen_rows -> dedup_rows -> select_rows -> rows_to_fastq give the host's texts,
    and screen_rows' tensors are the reference's, with the dtypes the docstrings name"""
    import numpy as np
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, trim_adapters, judge_rows, screen_index, screen_rows, dedup_rows, select_rows, rows_to_fastq, pack_names
    (t1, t2), contaminant = S.compose_text()
    ca, cj = S.compose_criteria()
    w1, w2, kept, counts = S.compose_expected(t1, t2, ca, cj, contaminant)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    ca = {k: v for k, v in ca.items() if k != "hist_len"}
    cj = dict(cj); flags = cj.pop("cut_flags")
    import _judge as J
    cj.update(cut_front=bool(flags & J.FRONT), cut_right=bool(flags & J.RIGHT), cut_tail=bool(flags & J.TAIL))
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        ix = screen_index(codec, [contaminant.decode()], k=S.COMPOSE_K)
        ix2 = screen_index(codec, pack_names([contaminant, b"", contaminant[:100].lower()], dev), k=S.COMPOSE_K)
        cut = trim_adapters(codec, t, codes=False, **ca)
        tc = dict(t, lens=cut["length"])
        j = judge_rows(codec, tc, codes=False, **cj)
        c = screen_rows(codec, tc, ix, pairs=True, codes=False, keep=j["keep"])
        c2 = screen_rows(codec, tc, ix2["index"], pairs=True, codes=False, keep=j["keep"].bool(), min_hits=3, min_pct=10, keep_matched=True)
        d = dedup_rows(codec, tc, pairs=True, keep=c["keep"])
        s = select_rows(codec, t, keep=d["keep"], start=j["start"], length=j["length"], pairs=True, min_len=cj["min_len"])
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
    stream.synchronize()
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2 and int(s["lens"].numel()) == 2 * kept
    model, npos = S.ref_set([contaminant], S.COMPOSE_K)
    for x in (ix, ix2):
        assert x["k"] == S.COMPOSE_K and x["n_kmers"] == len(model) == x["summary"]["n_kmers"] and x["slots"] == 2048 and x["index"].dtype == torch.uint8
        assert x["index"].numel() == 64 + 8 * 2048 == x["summary"]["index_bytes"]
    assert ix["summary"]["n_positions"] == npos and ix2["summary"]["n_refs"] == 3 and ix2["summary"]["ref_bases"] == 800
    B, lens, cand = (x.cpu().numpy() for x in (t["bases"], cut["length"], j["keep"]))
    for got, e in ((c, S.expected(B, lens, model, S.COMPOSE_K, False, pairs=True, cand=cand)),
                   (c2, S.expected(B, lens, model, S.COMPOSE_K, False, pairs=True, cand=cand, min_hits=3, min_pct=10, keep_matched=True))):
        for k in ("keep", "hits", "kmers"):
            assert np.array_equal(got[k].cpu().numpy().astype(np.int64), e[k].astype(np.int64)), k
        assert got["summary"] == e["summary"]
    assert c["summary"]["n_matched"] == counts["matched"] and d["summary"]["n_dups"] == counts["dups"]
    assert c["keep"].dtype == torch.uint8 and c["hits"].dtype == torch.int32 and c["kmers"].dtype == torch.int32


def test_screen_index_of_references_without_bytes(codec):
    """a list of only empty references is an empty set, not an error: every screen reports 0 hits"""
    import torch
    from repaq_amd.tensors import screen_index, screen_rows
    dev = torch.device("cuda:0")
    t = {"bases": torch.randint(0, 4, (6, 40), dtype=torch.uint8, device=dev), "lens": torch.full((6,), 40, dtype=torch.int32, device=dev)}
    for refs, n_refs in (([""], 1), ([b"", b""], 2), ([], 0), (["ACG", ""], 2)):
        ix = screen_index(codec, refs, k=16)
        assert ix["n_kmers"] == 0 and ix["slots"] == 1024 and ix["summary"]["n_refs"] == n_refs and ix["summary"]["ref_bases"] == sum(len(r) for r in refs)
        c = screen_rows(codec, t, ix)
        assert c["summary"]["hits"] == 0 and c["summary"]["kmers"] == 6 * 25 and bool(c["keep"].all())


# ---- 9: more units than a step of the LDS placement's capped grid
def test_many_short_rows_take_several_steps(codec):
    S.check_many_rows(codec)


# ---- 8: contention in the build
def test_hot_slots_in_the_build(codec):
    """65,536 x A: every lane of the build goes for ONE slot; a 4,096-base reference 16 times over: sixteen lanes for every slot, from many workgroups at a time.
    n_kmers has to be 1 and the model's count, both times, and the rows' outputs the model's, both times: whichever lane claims a slot, the set is the same.  (A
    condition the tree meets every time, not a rate.)"""
    import numpy as np
    rng = np.random.default_rng(66)
    k = 25
    unit = S.rand_seq(rng, 4096)
    seqs = [b"A" * 60, b"T" * 40 + S.rand_seq(rng, 20), unit[100:160], S.revcomp(unit[4000:4060]), unit[-30:] + unit[:30], S.rand_seq(rng, 60)]
    B, lens = S.rows_of(seqs, 64, "ascii")
    for refs, n_kmers in (([b"A" * 65536], 1), ([unit * 16], None), ([unit] * 16, None)):
        idx = S.Index(codec, refs, k)                                         # (the build's counts are compared with the model's in there)
        try:
            assert n_kmers is None or idx.result["n_kmers"] == n_kmers
            e = S.check(codec, B, lens, idx, what="hot slots")
            assert idx.build() == idx.result
            first = None
            dev = S.dev_rows(codec, B, lens)
            try:
                for _ in range(2):
                    out, summ, raw = S.run(codec, dev, idx)
                    S.compare(out, summ, e, "hot slots, after the second build:")
                    assert first is None or first == raw
                    first = raw
            finally:
                dev.free()
            assert e["summary"]["hits"] > 0
        finally:
            idx.free()
