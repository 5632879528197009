"""GPU (MI355X): the Python layer of repaq_amd.tensors on the product library - what every public function does BEFORE and AROUND its library calls: a malformed
tensor is refused by an assertion before the codec is touched, the context is on torch's stream for exactly the calls and back on its own afterwards, however they
end, rows without names stay without names, and name offsets keep the caller's dtype.  4 rows (2 pairs) at L = 16 with names of 2 and 3 bytes; what the calls
compute is the business of the other test_gpu_* files."""
import pytest

import _engine as E


pytestmark = pytest.mark.gpu

N, L = 4, 16


def _recording(name, fn):
    def method(self, *a, **kw):
        self.calls.append((name, a))
        return fn(self, *a, **kw)
    return method


def make_spy():
    """an RfqCodec that notes every call of a public method, in order, in .calls: (name, positional arguments)"""
    from repaq_amd import RfqCodec

    class Spy(RfqCodec):
        def __init__(self, *a, **kw):
            self.calls = []
            super().__init__(*a, **kw)

        def streams(self):
            return [a[0] for name, a in self.calls if name == "set_stream"]
    for name, fn in vars(RfqCodec).items():
        if callable(fn) and not name.startswith("_") and name != "close":
            setattr(Spy, name, _recording(name, fn))
    c = Spy(device=0, library=E.PRODUCT_LIB)
    assert "gfx950" in c.version()
    return c


@pytest.fixture(scope="module")
def codec():
    c = make_spy()
    yield c
    c.close()


@pytest.fixture(scope="module")
def rows(codec):
    """the rows every test here starts from (never changed), and what the calls without rows take: an image and a text of them, a screen index, a k-mer table"""
    import torch
    from repaq_amd import tensors as T
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(30)
    blob, off = T.pack_names([b"@a", b"@a", b"@bc", b"@bc"], dev)
    t = {"bases": torch.randint(0, 4, (N, L), dtype=torch.uint8, generator=g).to(dev), "quals": torch.tensor([[36], [30], [24], [12]], dtype=torch.uint8).repeat(1, L).to(dev),          # (the scores: one per row, so that any coder takes them)
         "lens": torch.tensor([16, 12, 16, 9], dtype=torch.int32, device=dev), "names": blob, "name_off": off}
    x = {"t": t, "dev": dev, "image": T.encode_tensors(codec, *_five(t)), "text": T.rows_to_fastq(codec, *_five(t)).clone(),
         "index": T.screen_index(codec, ["ACGTTGCAAGGCTTAGCCATGATC"], k=8), "table": T.kmer_table(codec, k=8, slots=1024),
         "bin": torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=dev), "insert": torch.tensor([20, -1], dtype=torch.int32, device=dev),
         "sample": torch.tensor([0, -1, 1, 0], dtype=torch.int32, device=dev)}
    T.count_kmers(codec, t, x["table"])
    torch.cuda.synchronize()
    return x


def _five(t):
    return tuple(t[k] for k in ("bases", "quals", "lens", "names", "name_off"))


def _rows_calls():
    """name -> (the call on (codec, x, t, **its per-row arguments), the per-row arguments it takes, the set_stream pairs one good call logs)"""
    from repaq_amd import tensors as T
    return {
        "select_rows": (lambda c, x, t, **kw: T.select_rows(c, t, **kw), ("keep", "start", "length"), 1),
        "group_rows": (lambda c, x, t, **kw: T.group_rows(c, t, x["bin"], 2, **kw), ("keep", "start", "length"), 1),
        "judge_rows": (lambda c, x, t: T.judge_rows(c, t, min_len=10), (), 1),
        "trim_adapters": (lambda c, x, t: T.trim_adapters(c, t, pairs=True, adapter1=b"AGATCGGAAGAGC"), (), 1),
        "merge_pairs": (lambda c, x, t: T.merge_pairs(c, t, x["insert"]), (), 2),
        "dedup_rows": (lambda c, x, t, **kw: T.dedup_rows(c, t, pairs=True, **kw), ("keep",), 1),
        "profile_rows": (lambda c, x, t, **kw: T.profile_rows(c, t, pairs=True, **kw), ("keep", "start", "length"), 1),
        "screen_rows": (lambda c, x, t, **kw: T.screen_rows(c, t, x["index"], **kw), ("keep",), 1),
        "count_kmers": (lambda c, x, t, **kw: T.count_kmers(c, t, x["table"], **kw), ("keep",), 1),
        "demux_rows": (lambda c, x, t, **kw: T.demux_rows(c, t, ["ACGT", "TTGA"], **kw), ("keep",), 1),
        "split_rows": (lambda c, x, t, **kw: T.split_rows(c, t, x["sample"], 2, **kw), ("start", "length"), 3),
        "filter_rows": (lambda c, x, t: T.filter_rows(c, t, min_len=10), (), 2),
        "encode_tensors": (lambda c, x, t: T.encode_tensors(c, *_five(t)), (), 1),
        "rows_to_fastq": (lambda c, x, t: T.rows_to_fastq(c, *_five(t)), (), 1),
    }


def _other_calls():
    """the public functions that take no rows: name -> (the call on (codec, x), the set_stream pairs one good call logs)"""
    from repaq_amd import tensors as T
    return {
        "decode_tensors": (lambda c, x: T.decode_tensors(c, x["image"]), 1),
        "decode_tensors_names": (lambda c, x: T.decode_tensors(c, x["image"], names=True), 2),
        "decode_names": (lambda c, x: T.decode_names(c, x["image"]), 1),
        "fastq_to_tensors": (lambda c, x: T.fastq_to_tensors(c, x["text"]), 1),
        "screen_index": (lambda c, x: T.screen_index(c, [b"ACGTTGCAAGGC"], k=8), 1),
        "kmer_table": (lambda c, x: T.kmer_table(c, k=8, slots=1024), 1),
        "kmer_counts": (lambda c, x: T.kmer_counts(c, x["table"], hist_len=4, index=True), 1),
    }


ROWS_CALLS = ("select_rows", "group_rows", "judge_rows", "trim_adapters", "merge_pairs", "dedup_rows", "profile_rows", "screen_rows", "count_kmers", "demux_rows",
              "split_rows", "filter_rows", "encode_tensors", "rows_to_fastq")
OTHER_CALLS = ("decode_tensors", "decode_tensors_names", "decode_names", "fastq_to_tensors", "screen_index", "kmer_table", "kmer_counts")


def test_the_lists_name_every_public_function():
    """a new public function of tensors.py fails here until it is in one of the lists (pack_names and group_parts make no call)"""
    import inspect
    from repaq_amd import tensors as T
    public = {n for n, f in vars(T).items() if inspect.isfunction(f) and f.__module__ == T.__name__ and not n.startswith("_")}
    assert public == (set(ROWS_CALLS) | set(OTHER_CALLS) | {"pack_names", "group_parts"}) - {"decode_tensors_names"}
    assert set(_rows_calls()) == set(ROWS_CALLS) and set(_other_calls()) == set(OTHER_CALLS)


# ---- 1: refusals come before any library call
@pytest.mark.parametrize("name", ROWS_CALLS)
def test_a_malformed_tensor_is_refused_before_any_call(codec, rows, name):
    import torch
    call, per_row, _ = _rows_calls()[name]
    t, dev = rows["t"], rows["dev"]
    bad = [("bases as int8", dict(t, bases=t["bases"].to(torch.int8)), {}),
           ("bases not contiguous", dict(t, bases=t["bases"][:, ::2]), {}),
           ("lens as int64", dict(t, lens=t["lens"].to(torch.int64)), {}),
           ("lens with n + 1 entries", dict(t, lens=torch.zeros((N + 1,), dtype=torch.int32, device=dev)), {}),
           ("lens on the CPU", dict(t, lens=t["lens"].cpu()), {})]
    if "keep" in per_row:
        bad += [("keep with n - 1 entries", t, {"keep": torch.ones((N - 1,), dtype=torch.uint8, device=dev)}),
                ("a float keep", t, {"keep": torch.ones((N,), dtype=torch.float32, device=dev)})]
    if "start" in per_row:
        bad += [("start as int64", t, {"start": torch.zeros((N,), dtype=torch.int64, device=dev)}),
                ("length as int64", t, {"length": torch.full((N,), 5, dtype=torch.int64, device=dev)})]
    for what, tt, kw in bad:
        codec.calls.clear()
        with pytest.raises(AssertionError):
            call(codec, rows, tt, **kw)
        assert codec.calls == [], "%s, %s: refused after %s" % (name, what, codec.calls)


# ---- 2: the scope is balanced
def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int64) if a.dtype == torch.uint64 else a,
                                                                                                  b.view(torch.int64) if b.dtype == torch.uint64 else b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def _stream(dev, side):
    import torch
    return torch.cuda.Stream(device=dev) if side else torch.cuda.current_stream(dev)


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("name", ROWS_CALLS + OTHER_CALLS)
def test_one_good_call_is_on_torch_s_stream_and_back(codec, rows, name, side_stream):
    import torch
    if name in ROWS_CALLS:
        call, _, pairs = _rows_calls()[name]
        args = (codec, rows, rows["t"])
    else:
        call, pairs = _other_calls()[name]
        args = (codec, rows)
    stream = _stream(rows["dev"], side_stream)
    stream.wait_stream(torch.cuda.current_stream(rows["dev"]))
    codec.calls.clear()
    with torch.cuda.stream(stream):
        call(*args)
    stream.synchronize()
    assert codec.streams() == [stream.cuda_stream, None] * pairs, codec.calls
    # every call of the library lies inside a pair: the first and the last thing the codec hears is the stream
    assert codec.calls[0][0] == "set_stream" and codec.calls[-1] == ("set_stream", (None,))


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("name", ["judge_rows", "select_rows"])
def test_a_call_the_library_refuses_ends_on_the_context_s_own_stream(codec, rows, name, side_stream):
    import torch
    from repaq_amd import RfqError
    from repaq_amd import tensors as T
    t = rows["t"]
    good, refused = {"judge_rows": (lambda: T.judge_rows(codec, t, cut_tail=True, cut_window=4, cut_mean_q=20), lambda: T.judge_rows(codec, t, cut_tail=True, cut_window=0)),
                     "select_rows": (lambda: T.select_rows(codec, t, keep=t["lens"] >= 12), lambda: T.select_rows(codec, t, row_len=1))}[name]
    stream = _stream(rows["dev"], side_stream)
    stream.wait_stream(torch.cuda.current_stream(rows["dev"]))
    with torch.cuda.stream(stream):
        want = good()
        codec.calls.clear()
        with pytest.raises(RfqError):
            refused()
        log = codec.streams()
        got = good()
    stream.synchronize()
    assert log[0] == stream.cuda_stream and log[-1] is None and len(log) == 2, log
    assert _same(got, want)
    if name == "select_rows":
        assert got["lens"].tolist() == [16, 12, 16] and got["name_off"].tolist() == [0, 2, 4, 7]


# ---- 3: rows without names
def test_rows_without_names_come_back_without_names(codec, rows):
    from repaq_amd import tensors as T
    t = rows["t"]
    bare = {k: t[k] for k in ("bases", "quals", "lens")}
    keep = t["lens"] >= 12
    pairs_of = [(T.select_rows(codec, bare, keep=keep), T.select_rows(codec, t, keep=keep)),
                (T.group_rows(codec, bare, rows["bin"], 2), T.group_rows(codec, t, rows["bin"], 2))]
    mb, mn = T.merge_pairs(codec, bare, rows["insert"]), T.merge_pairs(codec, t, rows["insert"])
    pairs_of += [(mb["merged"], mn["merged"]), (mb["unmerged"], mn["unmerged"])]
    assert mb["summary"] == dict(mn["summary"], names_len=0, max_name=0) and int(mn["merged"]["lens"].numel()) == 1 and int(mn["unmerged"]["lens"].numel()) == 2
    for got, named in pairs_of:
        assert "names" not in got and "name_off" not in got and "names" in named and "name_off" in named
        assert set(named) - set(got) == {"names", "name_off"}
        for k in got:
            assert _same(got[k], named[k]), k


# ---- 4: name offsets keep the caller's dtype
def test_uint64_name_offsets_stay_uint64(codec, rows):
    import torch
    from repaq_amd import tensors as T
    t = rows["t"]
    keep = t["lens"] >= 12
    s64 = T.select_rows(codec, t, keep=keep)
    su = T.select_rows(codec, dict(t, name_off=t["name_off"].view(torch.uint64)), keep=keep)
    assert s64["name_off"].dtype == torch.int64 and su["name_off"].dtype == torch.uint64
    assert su["name_off"].view(torch.int64).tolist() == s64["name_off"].tolist() == [0, 2, 4, 7]
    for k in ("bases", "quals", "lens", "names"):
        assert torch.equal(su[k], s64[k]), k
