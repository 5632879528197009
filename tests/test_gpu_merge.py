"""GPU (MI355X): rfq_merge_rows and repaq_amd.tensors.merge_pairs on the product library - every pair with an insert size to one row, the consensus of both mates,
under R1's name - against plain loops over the fragment's positions on the host (tests/_merge.py).  The CPU twin is tests/test_emu_merge.py."""
import numpy as np
import pytest

import _adapter as A
import _engine as E
import _merge as M

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
@pytest.mark.parametrize("row_len", M.ROW_LENS)
def test_shapes(codec, row_len):
    M.check_shapes(codec, row_len)


# ---- 2: every insert
@pytest.mark.parametrize("lengths", M.EVERY_INSERT_IDS)
def test_every_insert(codec, lengths):
    M.check_every_insert(codec, lengths)


# ---- 3: the consensus table
@pytest.mark.parametrize("codes", [True, False], ids=["codes", "ascii"])
def test_consensus_table(codec, codes):
    M.check_consensus_table(codec, codes)


# ---- 4: an oracle that does not share the rule's code
def test_fragments_come_back(codec):
    M.check_fragments(codec)


def test_fragments_come_back_with_tensors(codec):
    """test 4 through the tensors: trim_adapters(pairs=True) finds the inserts, merge_pairs gives the fragments back"""
    import torch
    from repaq_amd.tensors import trim_adapters, merge_pairs
    B, Q, lens, names, F = M.fragments()
    dev = torch.device("cuda:0")
    t = {"bases": torch.from_numpy(B).to(dev), "quals": torch.from_numpy(Q).to(dev), "lens": torch.from_numpy(lens).to(dev)}
    c = M.FRAG_CRIT
    a = trim_adapters(codec, t, pairs=True, min_overlap=c["min_overlap"], max_diff=c["max_diff"], max_diff_pct=c["max_diff_pct"])
    m = merge_pairs(codec, t, a["insert"], unmerged=False)
    insert = a["insert"].cpu().numpy(); diff = a["diff"].cpu().numpy()
    e = M.expected(B, Q, lens, None, insert, True)
    assert set(m) == {"merged", "summary"} and set(m["merged"]) == {"bases", "quals", "lens"}
    assert np.array_equal(m["merged"]["lens"].cpu().numpy(), insert[insert >= 0]) and m["summary"] == dict(zip(M.FIELDS, e["result"]))
    M.check_fragments_result(F, insert, diff, e, m["merged"]["bases"].cpu().numpy())


# ---- 5: nothing, everything, degenerate
def test_degenerate(codec):
    M.check_degenerate(codec)


# ---- 6: names
def test_names(codec):
    M.check_names(codec)


# ---- 7: outputs
def test_outputs_and_caps(codec):
    M.check_outputs(codec)


# ---- 8: refusals
def test_refused_on_the_host(codec):
    M.check_host_refusals(codec)


@pytest.mark.parametrize("label", M.DEVICE_REFUSALS)
def test_refused_on_the_device(codec, label):
    M.check_device_refusal(codec, label)


# ---- 9: the switch and the timings
def test_the_switch_and_the_stage_times(codec):
    M.check_switch_and_timings(codec)


# ---- 10: text -> adapter -> merge -> text
def test_text_adapter_merge_text(codec):
    M.check_composition(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_merge_pairs_with_tensors(codec, side_stream):
    """the composition's two texts through fastq_to_tensors -> trim_adapters -> merge_pairs -> rows_to_fastq of the merged rows and of the pairs that are not merged
    give the host's texts; every pair is in exactly one of the two"""
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, trim_adapters, merge_pairs, rows_to_fastq
    t1, t2 = A.compose_text()
    merged, w1, w2, n_merged, ea = M.compose_expected(t1, t2)
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    ca = M.COMPOSE_A
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        r = trim_adapters(codec, t, pairs=True, codes=False, min_overlap=ca["min_overlap"], max_diff=ca["max_diff"], max_diff_pct=ca["max_diff_pct"])
        m = merge_pairs(codec, t, r["insert"], codes=False)
        mg, um = m["merged"], m["unmerged"]
        g = rows_to_fastq(codec, mg["bases"], mg["quals"], mg["lens"], mg["names"], mg["name_off"], codes=False)
        g1, g2 = rows_to_fastq(codec, um["bases"], um["quals"], um["lens"], um["names"], um["name_off"], paired=PE_TWO_FILES, codes=False)
    stream.synchronize()
    assert np.array_equal(r["insert"].cpu().numpy(), ea["insert"])
    assert bytes(g.cpu().numpy().tobytes()) == merged, "the merged text differs from the host's"
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2, "the texts of the pairs that are not merged differ from the host's"
    pairs = int(t["lens"].numel()) // 2
    assert int(mg["lens"].numel()) == n_merged and int(mg["lens"].numel()) + int(um["lens"].numel()) // 2 == pairs == m["summary"]["n_pairs"]
    assert mg["lens"].dtype == torch.int32 and mg["name_off"].dtype == torch.int64 and mg["bases"].dtype == torch.uint8 and mg["quals"].dtype == torch.uint8
    assert um["lens"].dtype == torch.int32 and um["name_off"].dtype == torch.int64
    assert m["summary"]["n_rows"] == n_merged and m["summary"]["max_len"] == int(mg["bases"].shape[1])
