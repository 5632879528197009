"""GPU (MI355X): rfq_select_rows with a tag (rfq_name_tag) and repaq_amd.tensors.select_rows(tag=...) / extract_umi on the product library - a tag of the read's own
bases written into the kept names, UMI extraction - against a plain Python loop over rows that builds every expected name (tests/_tag.py).  The CPU twin is
tests/test_emu_tag.py; the composition with the tensors lives only here."""
import pytest

import _engine as E
import _tag as G


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


# ---- 1: the place
@pytest.mark.parametrize("at", (G.AT_SPACE, G.AT_END), ids=("space", "end"))
def test_the_tag_goes_in_front_of_the_first_space_or_to_the_end(codec, at):
    G.check_place(codec, at)


# ---- 2: the seams of the blob
@pytest.mark.parametrize("out_shift", range(16))
def test_tags_across_group_and_tile_boundaries_at_every_alignment(codec, out_shift):
    G.check_blob_seams(codec, out_shift)


def test_more_than_256_names_start_in_a_tile_some_empty_and_untagged(codec):
    G.check_many_names_in_a_tile(codec)


# ---- 3: the parts
@pytest.mark.parametrize("codes", (False, True), ids=("ascii", "codes"))
def test_parts_of_every_length_at_every_start_and_at_the_end_of_the_buffer(codec, codes):
    G.check_parts(codec, codes)


# ---- 4: pairs
def test_pairs_share_one_tag_and_dropped_pairs_give_no_name(codec):
    G.check_pairs(codec)


# ---- 5: identity
def test_a_tag_of_empty_parts_is_the_plain_call(codec):
    G.check_identity(codec)


# ---- 6: sizes
def test_size_query_short_cap_and_no_rows(codec):
    G.check_sizes(codec)


# ---- 7: refusals
def test_refused_on_the_host(codec):
    G.check_host_refusals(codec)


@pytest.mark.parametrize("label", G.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    G.check_device_refusal(codec, label)


# ---- 8: state
def test_tagged_plain_and_smaller_tagged_calls_follow_each_other(codec):
    G.check_state(codec)


def test_the_stages_of_a_tagged_call(codec):
    G.check_stage_names(codec)


# ---- 9: the switch
def test_the_switch_is_listed_and_resets(codec):
    G.check_option(codec, E.reset_options)


# ---- 10: composition with tensors
def _to_dev(b, dev):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)


def _names_of(t):
    blob = bytes(t["names"].cpu().numpy().tobytes()); off = [int(x) for x in t["name_off"].cpu()]
    return [blob[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("side_stream", [False, True])
def test_fastq_extract_umi_fastq_with_tensors(codec, side_stream):
    """two paired texts with inline UMIs through fastq_to_tensors -> extract_umi(per_read, 8 + 2 skipped, prefix UMI, pairs) -> rows_to_fastq give the model's two
    texts byte for byte (a read shorter than the UMI gives the shorter tag; a pair with a read the UMI used up is dropped); the same rows through encode_tensors ->
    decode_tensors(names=True) give back the tagged names"""
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, extract_umi, rows_to_fastq, encode_tensors, decode_tensors
    t1, t2 = G.compose_text()
    w1, w2, dropped, kept = G.compose_expected(t1, t2)
    _, _, none, kept0 = G.compose_expected(t1, t2, min_len=0)
    assert dropped >= 2 and none == 0 and len(t1[3][1]) == 5 and kept0[6] == t1[3][0][:-11] +b":UMI_" + t1[3][1] + b"_" + t2[3][1][:8] + b" 1:N:0:ACGT"
    dev = torch.device("cuda:0")
    a, b = _to_dev(G.fastq(t1), dev), _to_dev(G.fastq(t2), dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        s = extract_umi(codec, t, "per_read", 8, umi_skip=2, prefix="UMI", pairs=True, codes=False)
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
        codec.clearHeader()
        img = encode_tensors(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
        back = decode_tensors(codec, img, names=True)
        s0 = extract_umi(codec, t, "per_read", 8, umi_skip=2, prefix="UMI", pairs=True, codes=False, min_len=0)
    stream.synchronize()
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2
    assert s["dropped"]["short"] + s["dropped"]["mate"] == 2 * dropped and _names_of(s) == kept
    assert _names_of(back) == kept
    assert _names_of(s0) == kept0 and int(s0["lens"][6]) == 0, "a read shorter than the UMI gives the shorter tag"


@pytest.mark.parametrize("side_stream", [False, True])
def test_a_umi_behind_a_barcode_and_the_other_locations(codec, side_stream):
    """start=demux_rows(...)["start"]: the tag is the bases behind the barcode; loc read1 / read2 name one mate, which alone loses bases; code rows give letters.
    Every call and every torch op of extract_umi runs on the current stream or on a side stream; the comparisons follow its synchronisation"""
    import numpy as np
    import torch
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, demux_rows, extract_umi
    rng = np.random.default_rng(31)
    bcs = [b"ACGTACGT", b"TTGGCCAA", b"GATCGATC"]
    t1, t2 = [], []
    for p in range(40):
        recs = []
        for m in (1, 2):
            body = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(14, 40))))
            s = (b"GG" + bcs[p % 3] + b"T" + body) if m == 1 else body            # R1: 2 bases, the barcode, a linker base, then the UMI
            recs.append((b"@r%d %d:N:0" % (p, m), s, b"F" * len(s)))
        t1.append(recs[0]); t2.append(recs[1])
    dev = torch.device("cuda:0")
    a, b = _to_dev(G.fastq(t1), dev), _to_dev(G.fastq(t2), dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=True)
        dm = demux_rows(codec, t, bcs, pairs=True, off1=2, skip1=1, max_mm=0, codes=True)
        s = extract_umi(codec, t, "per_read", 6, umi_skip=1, start=dm["start"], pairs=True, codes=True)
        by_loc = {loc: extract_umi(codec, t, loc, 6, umi_skip=1, prefix="RX", sep="#", start=dm["start"], pairs=True, codes=True) for loc in ("read1", "read2")}
    stream.synchronize()
    assert int(dm["keep"].sum()) == 80 and int(dm["start"][0]) == 11 and int(dm["start"][1]) == 0
    starts = dm["start"].cpu().numpy()
    w1, w2, dropped, kept = G.compose_expected(t1, t2, umi_len=6, umi_skip=1, prefix=b"", starts=starts)
    assert dropped == 0 and kept[0] == b"@r0:" + t1[0][1][11:17] + b"_" + t2[0][1][:6] + b" 1:N:0" and _names_of(s) == kept
    lens = t["lens"].cpu().numpy()
    assert np.array_equal(s["lens"].cpu().numpy(), lens - starts - 7)
    for loc, mate in (("read1", 0), ("read2", 1)):
        s = by_loc[loc]
        want = []
        for p in range(40):
            src = (t1, t2)[mate][p][1]; a = int(starts[2 * p + mate])
            for m in (0, 1):
                name = (t1, t2)[m][p][0]; at = name.index(b" ")
                want.append(name[:at] + b"#RX_" + src[a:a + 6] + name[at:])
        cut = np.where(np.arange(80) % 2 == mate, 7, 0)
        assert _names_of(s) == want and np.array_equal(s["lens"].cpu().numpy(), lens - starts - cut)
    with pytest.raises(AssertionError):
        extract_umi(codec, t, "read2", 6, codes=True)


def test_an_empty_batch_takes_a_tag_as_it_takes_the_plain_call(codec):
    """no rows: an empty tensor has no pointer to hand over, so the tag's arrays arrive as NULL - select_rows(tag=...) and extract_umi give the empty rows the plain
    call gives, on both formulations"""
    import torch
    from repaq_amd.tensors import select_rows, extract_umi, pack_names
    dev = torch.device("cuda:0")
    blob, off = pack_names([], dev)
    t = {"bases": torch.empty((0, 24), dtype=torch.uint8, device=dev), "quals": torch.empty((0, 24), dtype=torch.uint8, device=dev),
         "lens": torch.empty((0,), dtype=torch.int32, device=dev), "names": blob, "name_off": off}
    plain = select_rows(codec, t)
    for path in G.PATHS:
        codec.set_option(G.OPTION, path)
        for pairs in (False, True):
            for got in (select_rows(codec, t, pairs=pairs, tag=dict(start=t["lens"], length=t["lens"], prefix="UMI")),
                        extract_umi(codec, t, "per_read" if pairs else "read1", 8, umi_skip=2, prefix="UMI", pairs=pairs)):
                assert got["dropped"] == plain["dropped"] == {"mask": 0, "short": 0, "mate": 0}
                for k in ("bases", "quals", "lens", "names", "name_off"):
                    assert got[k].shape == plain[k].shape and got[k].dtype == plain[k].dtype and torch.equal(got[k], plain[k]), k
        assert plain["name_off"].tolist() == [0] and plain["lens"].numel() == 0
