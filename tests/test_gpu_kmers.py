"""GPU (MI355X): rfq_kmers_init, rfq_kmers_rows, rfq_kmers_read and repaq_amd.tensors.kmer_table / count_kmers / kmer_counts on the product library - rows to a
caller-owned table of canonical k-mers with counts that adds up across calls, and the table to its spectrum, its (value, count) list and a screen index - against a
collections.Counter made by a plain loop over the positions (tests/_kmers.py).  The CPU twin is tests/test_emu_kmers.py; the repeated runs of the hot values, the
many-rows walk and the tensors live only here."""
import pytest

import _engine as E
import _kmers as K

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
@pytest.mark.parametrize("k", K.KS)
def test_a_planted_kmer_at_every_position(codec, k):
    K.check_every_position(codec, k)


# ---- 2: validity
def test_other_bytes_short_rows_padding_and_a_palindrome(codec):
    K.check_validity(codec)


# ---- 3: seams
@pytest.mark.parametrize("row_len", K.S.SEAM_IDS)
def test_kmers_across_lane_kernel_and_tile_seams(codec, row_len):
    K.check_seams(codec, row_len)


@pytest.mark.parametrize("case", K.W.WALK_IDS)
def test_walk_seams(codec, case):
    K.check_walk(codec, case)


def test_walk_bad_length_in_the_last_row(codec):
    K.check_walk_bad_length(codec)


def test_many_short_rows_take_more_steps_than_the_least(codec):
    """more rows than KM_ITER steps of a grid of eight workgroups per compute unit hold, so that a workgroup takes more steps and the last one is part empty; the
    rows are 997 distinct ones in a fixed order: the model counts those, the table's counts are theirs times how often each comes"""
    import collections
    import numpy as np
    S = K.S
    n, k, L, D = 200_006, 15, 48, 997
    rng = np.random.default_rng(87)
    seqs = [S.rand_seq(rng, int(rng.integers(0, L + 1))) for _ in range(D)]
    Bd, ld = S.rows_of(seqs, L, "code")
    pick = (np.arange(n, dtype=np.int64) * 7 + np.arange(n, dtype=np.int64) // D) % D
    times = np.bincount(pick, minlength=D)
    cnt = collections.Counter(); kd = np.zeros(D, np.uint32)
    for i in range(D):
        c = collections.Counter(S.kmers_of(S.digits(Bd[i, :ld[i]].tobytes(), True), k))
        kd[i] = sum(c.values())
        for v, x in c.items():
            cnt[v] += x * int(times[i])
    B, lens = np.ascontiguousarray(Bd[pick]), ld[pick]
    dev = S.dev_rows(codec, B, lens)
    try:
        for path in (None, "direct"):
            t = K.Table(codec, k, 2 * len(cnt))
            try:
                codec.set_option(K.OPTION, path)
                got, summ, _ = t.count(dev, codes=True)
                codec.set_option(K.OPTION, None)
                assert np.array_equal(got, kd[pick])
                assert summ == dict(n_rows=n, n_counted=n, bases_in=int(lens.sum()), added=sum(cnt.values()), n_new=len(cnt), n_kmers=len(cnt), total=sum(cnt.values()), lost=0)
                t.check(cnt=cnt, what="many rows under %s" % (path or "default"))
            finally:
                t.free()
    finally:
        dev.free()


# ---- 4: adding up
def test_calls_add_up_in_any_order_masks_cut_lengths_and_the_screens_kmers(codec):
    K.check_adding_up(codec)


# ---- 5: hot values
def test_hot_values_twice_into_fresh_tables(codec):
    K.check_hot(codec, twice=True, paths=K.PATHS)


# ---- 6: formulations
def test_default_general_direct_and_collide_agree(codec):
    K.check_formulations(codec, labels=K.S.SEAM_IDS)


def test_the_switch_is_listed_and_resets(codec):
    K.check_option(codec, E.reset_options)


# ---- 7: the read
def test_read_selection_spectrum_room_and_the_index(codec):
    K.check_read(codec)


# ---- 8: a table that is full
def test_a_full_table_is_refused_marked_and_formatted_again(codec):
    K.check_full(codec)


# ---- 9: refusals
def test_init_refused(codec):
    K.check_init_refusals(codec)


def test_rows_and_read_refused_on_the_host(codec):
    K.check_host_refusals(codec)


def test_a_table_that_is_none_and_a_table_of_garbage(codec):
    K.check_bad_table(codec)


@pytest.mark.parametrize("label", K.DEVICE_REFUSAL_IDS)
def test_refused_on_the_device(codec, label):
    K.check_device_refusal(codec, label)


# ---- 10: state and composition
def test_a_count_leaves_other_calls_alone(codec):
    K.check_state(codec)


@pytest.mark.parametrize("side_stream", [False, True])
def test_adapter_judge_count_read_screen_select_with_tensors(codec, side_stream):
    """two small texts through fastq_to_tensors -> trim_adapters -> judge_rows -> count_kmers(keep = the judge's) -> kmer_counts(min_count=2, index=True) ->
    screen_rows(keep_matched, min_pct=50) -> select_rows -> rows_to_fastq give the host's texts; the tensors are the model's, with the dtypes the docstrings name"""
    import numpy as np
    import torch
    import _adapter as A
    import _judge as J
    from repaq_amd import PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, trim_adapters, judge_rows, kmer_table, count_kmers, kmer_counts, screen_rows, select_rows, rows_to_fastq
    S = K.S
    t1, t2 = K.compose_texts()
    ca, cj = S.compose_criteria()
    w1, w2, kept, cnt, kmers, cut_w, keep_w = K.compose_expected(t1, t2, ca, cj)
    sel = K.selected(cnt, 2)
    assert 10 < kept < len(t1) and len(sel) > 100 and len(sel) < len(cnt), (kept, len(sel), len(cnt))
    dev = torch.device("cuda:0")
    a = torch.frombuffer(bytearray(b"".join(t1)), dtype=torch.uint8).to(dev); b = torch.frombuffer(bytearray(b"".join(t2)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(device=dev) if side_stream else torch.cuda.current_stream(dev)
    ca = {k: v for k, v in ca.items() if k != "hist_len"}
    cj = dict(cj); flags = cj.pop("cut_flags")
    cj.update(cut_front=bool(flags & J.FRONT), cut_right=bool(flags & J.RIGHT), cut_tail=bool(flags & J.TAIL))
    with torch.cuda.stream(stream):
        t = fastq_to_tensors(codec, a, b, paired=PE_TWO_FILES, codes=False)
        cut = trim_adapters(codec, t, codes=False, **ca)
        tc = dict(t, lens=cut["length"])
        j = judge_rows(codec, tc, codes=False, **cj)
        tab = kmer_table(codec, k=K.COMPOSE_K, slots=2 * len(cnt))
        half = tc["lens"].numel() // 2 & ~1
        c1 = count_kmers(codec, {"bases": tc["bases"][:half], "lens": tc["lens"][:half]}, tab, codes=False, keep=j["keep"][:half])
        c2 = count_kmers(codec, {"bases": tc["bases"][half:], "lens": tc["lens"][half:]}, tab["table"], codes=False, keep=j["keep"][half:].bool())
        kc = kmer_counts(codec, tab, min_count=2, hist_len=8, index=True)
        every = kmer_counts(codec, tab["table"])
        sc = screen_rows(codec, tc, kc["index"], pairs=True, codes=False, keep=j["keep"], keep_matched=True, min_pct=50)
        s = select_rows(codec, t, keep=sc["keep"], start=j["start"], length=j["length"], pairs=True, min_len=cj["min_len"])
        g1, g2 = rows_to_fastq(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES, codes=False)
    stream.synchronize()
    assert np.array_equal(cut["length"].cpu().numpy(), cut_w) and np.array_equal(j["keep"].cpu().numpy(), keep_w)
    assert np.array_equal(torch.cat([c1["kmers"], c2["kmers"]]).cpu().numpy().astype(np.int64), kmers.astype(np.int64))
    assert c2["summary"]["n_kmers"] == len(cnt) and c2["summary"]["total"] == sum(cnt.values()) and c1["summary"]["n_new"] + c2["summary"]["n_new"] == len(cnt)
    assert list(zip(kc["values"].tolist(), kc["counts"].tolist())) == sel
    assert list(zip(every["values"].tolist(), every["counts"].tolist())) == K.selected(cnt) and every["hist"] is None and every["index"] is None
    assert np.array_equal(kc["hist"].cpu().numpy().astype(np.uint64), K.spectrum(cnt, 8))
    assert kc["summary"]["n_selected"] == len(sel) and kc["index"]["n_kmers"] == len(sel) and kc["index"]["k"] == K.COMPOSE_K
    assert kc["index"]["index"].numel() == 64 + 8 * kc["index"]["slots"] == kc["summary"]["index_bytes"]
    assert bytes(g1.cpu().numpy().tobytes()) == w1 and bytes(g2.cpu().numpy().tobytes()) == w2 and int(s["lens"].numel()) == 2 * kept
    assert tab["table"].dtype == torch.uint8 and c1["kmers"].dtype == torch.int32 and kc["values"].dtype == torch.int64 and kc["counts"].dtype == torch.int64
    assert kc["hist"].dtype == torch.int64 and kc["index"]["index"].dtype == torch.uint8
