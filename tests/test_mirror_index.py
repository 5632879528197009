"""Two-file PE through ONE line index (RFQ_MIRROR, default on): where both files have the same size the encoder indexes R1 only and reads R2 through R1's
line table; k_gather2 proves, record by record, that R2's line feeds sit where the table says (and that it holds no '\\r'), k_mirror_tail does the same for the text
behind the last encoded unit, and a mismatch (DE_MIRROR_FAIL, never seen by the caller) repeats the batch with an index per file.

Every case: two files at -k 100 (a few hundred pairs make several chunks); the image and consumed1/2 equal _oracle.encode_file and what a context with
RFQ_MIRROR=0 returns (its error, where the text is broken); the path taken is read from the timings() markers - `mirror_index`: one index served both files;
`mirror_fallback`: a batch of this call was repeated with both.  A case that expects the fallback asserts its marker: it never passes as "mirrored and happened
to be equal".  Each case runs on the SIMT interpreter (tests/emu, CPU) and, marked gpu, on the product library."""
import pytest

import _engine as E
import _oracle as O

CB = 100_000                                    # -k 100
PAIRS = {O.NOVA_PE150: 700, O.BGI_PE100: 1100}  # two whole chunks and a part of the third


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def make(request):
    from repaq_amd import RfqCodec
    if request.param == "gpu":
        import torch
        assert torch.cuda.is_available()
        lib, tag = E.PRODUCT_LIB, "gfx950"
    else:
        lib, tag = E.build_emu(), "simt-emulation"
    made = []

    def make_codec(mirror=True):
        c = RfqCodec(device=0, library=lib)
        assert tag in c.version()
        E.reset_options(c)                      # (whatever the environment says)
        if not mirror:
            c.set_option("RFQ_MIRROR", "0")
        made.append(c)
        return c
    yield make_codec
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def off(make):
    """the context every case compares with: an index per file, always"""
    return make(mirror=False)


@pytest.fixture()
def on(make):
    """a fresh context per case: what a mismatch leaves behind must not reach the next one"""
    return make()


_INPUTS = {}


def pe(profile=O.NOVA_PE150, seed=3):
    """(fq1, fq2, oracle image) of a generated pair of files - made once, never changed"""
    key = (profile, seed)
    if key not in _INPUTS:
        fq1, fq2 = O.gen(profile, PAIRS[profile], seed=seed, **(dict(n_quals=40) if profile == O.BGI_PE100 else {}))
        assert len(fq1) == len(fq2) and nl_pos(fq1) == nl_pos(fq2)
        _INPUTS[key] = (fq1, fq2, O.encode_file(fq1, fq2, O.PE_TWO_FILES, CB))
    return _INPUTS[key]


def nl_pos(b):
    return [i for i, c in enumerate(b) if c == 10]


def records(fq):
    ln = fq.split(b"\n")
    assert ln[-1] == b""
    return [ln[i:i + 4] for i in range(0, len(ln) - 1, 4)]


def text(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def run(codec, fq1, fq2, paired=O.PE_TWO_FILES, clear=True, whole=None, **kw):
    """one rfq_encode_batch call -> (error code or 0, error text, image, consumed1, consumed2, n_reads) and the call's markers.  whole: the files this text is a
    part of (the line-break thresholds are the file's)"""
    from repaq_amd import RfqError
    if clear:
        codec.clearHeader()
    d1 = codec.dev_put(fq1); d2 = codec.dev_put(fq2) if paired == O.PE_TWO_FILES else None
    try:
        args = dict(E.nolb_args(*(whole or (fq1, fq2)), paired)); args.update(kw)
        try:
            r = codec.encode(d1, len(fq1), d2, len(fq2) if d2 else 0, paired, CB, **args)
            out = (0, "", codec.dev_get(r.d_rfq, r.rfq_len) if r.rfq_len else b"", r.consumed1, r.consumed2, r.n_reads)
        except RfqError as e:
            out = (e.code, e.message, b"", 0, 0, 0)
        return out, {n for n, _ in codec.timings()}
    finally:
        codec.dev_free(d1)
        if d2:
            codec.dev_free(d2)


def mirrored(marks):
    return "mirror_index" in marks and "mirror_fallback" not in marks


def fell_back(marks):
    return "mirror_fallback" in marks and "mirror_index" not in marks


def untouched(marks):
    return "mirror_index" not in marks and "mirror_fallback" not in marks


def check_fallback(on, off, fq1, fq2, want=None, **kw):
    """a text whose mates do not share their line ends: the batch is repeated with both indexes and the result is the RFQ_MIRROR=0 context's (and the oracle's, where
    it has one)"""
    ref, m0 = run(off, fq1, fq2, **kw)
    assert untouched(m0), sorted(m0)
    got, m = run(on, fq1, fq2, **kw)
    assert fell_back(m), sorted(m)
    assert got == ref, (got[:2], ref[:2], got[3:], ref[3:])
    if want is not None:
        assert got[:3] == (0, "", want) and got[3:5] == (len(fq1), len(fq2))
    return got


# ---------------------------------------------------------------- 1, 2: mates whose lines coincide
@pytest.mark.parametrize("profile", [O.NOVA_PE150, O.BGI_PE100], ids=["nova150", "bgi100_q40"])
def test_coinciding_mates_are_indexed_once(on, off, profile):
    fq1, fq2, want = pe(profile)
    got, m = run(on, fq1, fq2)
    assert mirrored(m), sorted(m)
    assert got[:5] == (0, "", want, len(fq1), len(fq2))
    ref, m0 = run(off, fq1, fq2)
    assert untouched(m0) and ref == got
    # a call that does not end the input leaves the part of a chunk behind; the next one takes it from there
    a, ma = run(on, fq1, fq2, final=False)
    assert mirrored(ma), sorted(ma)
    assert a == run(off, fq1, fq2, final=False)[0]
    assert a[0] == 0 and 0 < a[3] < len(fq1) and a[3] == a[4]
    b, mb = run(on, fq1[a[3]:], fq2[a[4]:], clear=False, whole=(fq1, fq2), emit_header=False, file_off1=a[3], file_off2=a[4])
    assert mirrored(mb), sorted(mb)
    assert b[0] == 0 and a[2] + b[2] == want


def test_coinciding_mates_without_their_last_line_feed(on, off):
    """both files end in an unterminated line: the table's last entry is the virtual terminator behind the text"""
    fq1, fq2, _ = pe()
    fq1, fq2 = fq1[:-1], fq2[:-1]
    got, m = run(on, fq1, fq2)
    assert mirrored(m), sorted(m)
    assert got[:5] == (0, "", O.encode_file(fq1, fq2, O.PE_TWO_FILES, CB), len(fq1), len(fq2)) and got == run(off, fq1, fq2)[0]


@pytest.mark.parametrize("clear", [True, False], ids=["clearHeader", "same_header"])
def test_repeated_encode_stays_mirrored(on, clear):
    fq1, fq2, want = pe()
    for call in range(3):
        got, m = run(on, fq1, fq2, clear=clear or call == 0)
        assert mirrored(m), (call, sorted(m))
        assert got[:5] == (0, "", want, len(fq1), len(fq2)), call


def test_less_than_a_chunk_is_not_taken_on_trust(on, off):
    """a call that does not end the input and holds no whole chunk: nothing was gathered, so nothing was proven - the empty result is the one of both indexes, and the
    context does not give up on the input"""
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1)[:100], records(fq2)[:100]
    got, m = run(on, text(r1), text(r2), final=False)
    assert got == run(off, text(r1), text(r2), final=False)[0] and got[2:5] == (b"", 0, 0)       # (an empty result collects no stage times: no marker to read)
    got, m = run(on, fq1, fq2, clear=False)
    assert mirrored(m), sorted(m)


# ---------------------------------------------------------------- 3, 4: the same bytes in all, other line ends
def _last_encoded_pair(off, fq1, fq2):
    (rc, _, _, c1, _, n_reads), _ = run(off, fq1, fq2, final=False)
    assert rc == 0 and n_reads
    return n_reads // 2 - 1


@pytest.mark.parametrize("where", ["first_of_chunk0", "mid_later_chunk", "last_encoded"])
def test_names_of_other_lengths_fall_back(on, off, where):
    """R2 with one name a byte longer and the next a byte shorter: the files' sizes are equal, two line ends are not where R1's are"""
    fq1, fq2, _ = pe()
    r2 = records(fq2); final = where != "last_encoded"
    k = {"first_of_chunk0": 0, "mid_later_chunk": 333 + 150, "last_encoded": _last_encoded_pair(off, fq1, fq2) - 1}[where]
    r2[k][0] += b"A"; r2[k + 1][0] = r2[k + 1][0][:-1]
    bad = text(r2)
    assert len(bad) == len(fq1) and nl_pos(bad) != nl_pos(fq1)
    got = check_fallback(on, off, fq1, bad, want=O.encode_file(fq1, bad, O.PE_TWO_FILES, CB) if final else None, final=final)
    assert got[0] == 0 and got[2]
    # the context remembers: the same input again (the header stays) is indexed twice without an attempt
    again, m = run(on, fq1, bad, clear=False, final=final)
    assert untouched(m), sorted(m)
    assert again == got
    # ... until the header is cleared: another input
    fq1, fq2, want = pe()
    got, m = run(on, fq1, fq2)
    assert mirrored(m) and got[2] == want


def test_reads_of_other_lengths_fall_back(on, off):
    """R2 with one read a base shorter and its neighbour a base longer, sequence and quality both"""
    fq1, fq2, _ = pe()
    r2 = records(fq2); k = 400
    r2[k][1] = r2[k][1][:-1]; r2[k][3] = r2[k][3][:-1]; r2[k + 1][1] += b"C"; r2[k + 1][3] += b"F"
    bad = text(r2)
    assert len(bad) == len(fq1)
    check_fallback(on, off, fq1, bad, want=O.encode_file(fq1, bad, O.PE_TWO_FILES, CB))


# ---------------------------------------------------------------- 5, 6: four line feeds per record, in the wrong places
def _move_line_feed(fq2, gone, put):
    """the line feed at offset `gone` becomes a letter, the byte at offset `put` a line feed"""
    b = bytearray(fq2)
    assert b[gone] == 10 and b[put] != 10
    b[gone] = ord("A"); b[put] = 10
    return bytes(b)


def _line_ends(fq, k):
    """offsets of the four line feeds of record k"""
    return nl_pos(fq)[4 * k:4 * k + 4]


def _record_start(fq, k):
    return ([-1] + nl_pos(fq))[4 * k] + 1


@pytest.mark.parametrize("k", [0, 450], ids=["chunk0", "chunk1"])
def test_line_feed_moved_inside_a_record(on, off, k):
    """the sequence line's end replaced by a letter, a byte of the quality line by a line feed: the record still has four line feeds"""
    fq1, fq2, _ = pe()
    ends = _line_ends(fq2, k)
    bad = _move_line_feed(fq2, ends[1], ends[2] + 40)
    check_fallback(on, off, fq1, bad)


@pytest.mark.parametrize("line", ["name_behind_byte_64", "strand"])
def test_line_feed_moved_where_only_the_count_looks(on, off, line):
    """the same in the part of a name behind its parsed 64 bytes, and in a '+' line that repeats the name: no lane has those bytes in its registers"""
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2); k = 380
    if line == "name_behind_byte_64":
        for r in (r1, r2):
            r[k][0] += b" " + b"x" * 60
    else:
        for r in (r1, r2):
            r[k][2] = b"+" + r[k][0][1:]
    a, b = text(r1), text(r2)
    assert nl_pos(a) == nl_pos(b)
    got, m = run(on, a, b)                                                   # (the edit itself keeps the mates aligned)
    assert mirrored(m) and got[:3] == (0, "", O.encode_file(a, b, O.PE_TWO_FILES, CB))
    ends = _line_ends(b, k); start = _record_start(b, k)
    bad = _move_line_feed(b, ends[0], start + 80) if line == "name_behind_byte_64" else _move_line_feed(b, ends[2], ends[1] + 20)
    check_fallback(on, off, a, bad)


# ---------------------------------------------------------------- 7: '\r'
def test_carriage_return_in_r2(on, off):
    """one line of R2 ends in '\\r\\n', a name a byte shorter keeps the sizes equal: the repeat's own index sees the '\\r' and the text is normalised, as without the mirror"""
    fq1, fq2, _ = pe()
    r2 = records(fq2); k = 300
    r2[k][1] += b"\r"; r2[k + 1][0] = r2[k + 1][0][:-1]
    bad = text(r2)
    assert len(bad) == len(fq1)
    check_fallback(on, off, fq1, bad, want=O.encode_file(fq1, bad, O.PE_TWO_FILES, CB))
    # '\r' in the place of a letter, every line feed where R1's is: the control-byte count alone
    b = bytearray(fq2); p = _record_start(fq2, k) + 100; b[p] = 13
    assert nl_pos(bytes(b)) == nl_pos(fq1)
    check_fallback(on, off, fq1, bytes(b))


# ---------------------------------------------------------------- 8, 9: behind the last encoded unit
def test_difference_behind_the_last_encoded_unit(on, off):
    """a call that does not end the input: the mates differ only in the records of the chunk that is not full yet (consumed2, and the next call, depend on them)"""
    fq1, fq2, _ = pe()
    k = _last_encoded_pair(off, fq1, fq2) + 5
    r2 = records(fq2)
    assert k + 1 < len(r2)
    r2[k][0] += b"A"; r2[k + 1][0] = r2[k + 1][0][:-1]
    bad = text(r2)
    got = check_fallback(on, off, fq1, bad, final=False)
    assert got[0] == 0 and got[2] and got[3] == got[4]


@pytest.mark.parametrize("which", ["r2", "r1"])
def test_last_line_feed_missing_in_one_file(on, off, which):
    """one file's last line feed replaced by a quality value (sizes equal): its last line is unterminated, the other's is not"""
    fq1, fq2, _ = pe()
    a, b = (fq1, fq2[:-1] + b"F") if which == "r2" else (fq1[:-1] + b"F", fq2)
    check_fallback(on, off, a, b)


@pytest.mark.parametrize("which", ["r2", "r1"])
@pytest.mark.parametrize("cut", ["no_last_line_feed", "truncated_record"])
def test_one_file_shorter_at_its_end(on, off, which, cut):
    """a file without its last line feed, or with its last record cut inside the sequence line: the sizes differ, both files are indexed, no attempt"""
    fq1, fq2, _ = pe()
    drop = 1 if cut == "no_last_line_feed" else 200
    a, b = (fq1, fq2[:-drop]) if which == "r2" else (fq1[:-drop], fq2)
    got, m = run(on, a, b)
    assert untouched(m), sorted(m)
    assert got == run(off, a, b)[0]


# ---------------------------------------------------------------- 10, 11, 12
def test_sizes_differ_no_attempt(on, off):
    fq1, fq2, _ = pe()
    r2 = records(fq2); r2[10][0] += b"A"
    bad = text(r2)
    got, m = run(on, fq1, bad)
    assert untouched(m), sorted(m)
    assert got[:5] == (0, "", O.encode_file(fq1, bad, O.PE_TWO_FILES, CB), len(fq1), len(bad)) and got == run(off, fq1, bad)[0]


def test_a_pair_longer_than_a_tile(on, off):
    """one pair of 2,500-base reads among mates that coincide: equal to the oracle, whichever path took it"""
    import random
    fq1, fq2, _ = pe()
    rng = random.Random(11); r1, r2 = records(fq1), records(fq2)
    for r in (r1, r2):
        r[350][1] = bytes(rng.choice(b"ACGT") for _ in range(2500)); r[350][3] = bytes(rng.choice(b"F:,") for _ in range(2500))
    a, b = text(r1), text(r2)
    assert nl_pos(a) == nl_pos(b)
    got, m = run(on, a, b)
    assert got[:5] == (0, "", O.encode_file(a, b, O.PE_TWO_FILES, CB), len(a), len(b)) and got == run(off, a, b)[0]
    assert mirrored(m) or fell_back(m), sorted(m)


def test_single_end_and_interleaved_are_untouched(on, off):
    fq1, fq2, _ = pe()
    got, m = run(on, fq1, b"", paired=O.SE)
    assert untouched(m) and got[:4] == (0, "", O.encode_file(fq1, b"", O.SE, CB), len(fq1)) and got == run(off, fq1, b"", paired=O.SE)[0]
    il, _ = O.gen(O.NOVA_PE150, 400, seed=6, interleaved=True)
    got, m = run(on, il, b"", paired=O.PE_INTERLEAVED)
    assert untouched(m) and got[:4] == (0, "", O.encode_file(il, b"", O.PE_INTERLEAVED, CB), len(il)) and got == run(off, il, b"", paired=O.PE_INTERLEAVED)[0]
