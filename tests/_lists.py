"""Test infrastructure: the smallest inputs at which the position-list passes of the fused decode (dec/pos_lists.h: k_dec_pos_sum2 with 16 stream bytes
per lane and 1024 per step, k_dec_pos_list with 4 and 256; segments of 1024 / 2048 / 4096 bytes, the N-position stream in the same launches) can go wrong.  A case is a hand-made single-end FASTQ - reads of 150, 'F' everywhere except where the
case puts ':' or ',' - whose ':' stream the case designs token by token (format: head comment of enc/pos_coder.h).  The oracle encodes it; the case reads its stream
back out of the image (tests/_sections.py) and asserts that it is byte for byte the designed one and that the bytes at the boundary it aims at are the intended
ones; then the library decodes the image under every RFQ_POS_SEG and the text must come back - on the fused path ("emit" among the stages, "emit_expanded" not).
Run by tests/test_emu_lists.py (SIMT interpreter) and tests/test_gpu_lists.py (MI355X); tools/lists_asan.sh decodes the same images under the host sanitizers."""
import functools
import os

import _oracle as O
import _sections as S

READ = 150
MAX_READS = 1300
SEGS = ("1024", "2048", "4096")
COLON, COMMA = ord(":"), ord(",")
EDGES = (16, 32, 1024, 2048, 4096)          # lane, lane, step (= the smallest segment), segment, segment edges of a stream
D2, D4 = 300, 17000                         # distances whose gap tokens take 2 and 4 bytes


def gap(d):
    """the gap token of distance d (d - 1 in 7, 14 or 29 bits)"""
    v = d - 1
    if v < 128:
        return bytes([v])
    if v < 16384:
        return bytes([0x80 | (v >> 8), v & 0xFF])
    return bytes([0xE0 | (v >> 24), (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF])


def model(items):
    """items: d (a lone position d behind the previous one) or (d, n) (a streak of n positions that starts there); every d but the first >= 2.
    -> positions, the stream that codes them, the stream offset of every item's first token and the offset behind its last"""
    pos, out, first, behind, prev = [], bytearray(), [], [], -1
    for it in items:
        d, n = it if isinstance(it, tuple) else (it, 1)
        a = prev + d; e = a + n - 1
        first.append(len(out)); out += gap(d)
        k = a + 1
        if a == 0 and n >= 2:
            out.append(0x00); k = 2
        while k <= e:
            r = min(32, e - k + 1); out.append(0xC0 | (r - 1)); k += r
        behind.append(len(out)); pos.extend(range(a, e + 1)); prev = e
    return pos, bytes(out), first, behind


def text(marks, n_at=(), reads=None):
    """the FASTQ: quality `value` at the text positions marks[value], 'N' bases at n_at (they carry the major quality like every other base)"""
    top = max([p for v in marks.values() for p in v] + list(n_at) + [0])
    n = reads or max(top // READ + 1, sum(map(len, marks.values())) // 50 + 1)      # ('F' stays the major value: at most a third of a read is marked)
    assert n <= MAX_READS and top < n * READ, (n, top)
    q = bytearray(b"F" * (READ * n)); s = bytearray((b"ACGT" * 38)[:READ] * n)
    for v, ps in marks.items():
        for p in ps:
            q[p] = v
    for p in n_at:
        s[p] = ord("N")
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(s[READ * i:READ * i + READ]), bytes(q[READ * i:READ * i + READ])) for i in range(n))


def designed(items, probes, comma=(4,), n_at=(), reads=None):
    """a one-chunk case whose ':' stream is model(items); probes: (stream offset, bytes expected there)"""
    pos, stream, _, _ = model(items)
    return dict(fq=text({COLON: pos, COMMA: [p for p in comma if p not in set(pos)]}, n_at, reads), chunk_bases=1_000_000, streams=[{COLON: stream}], probes=[(0, COLON, o, b) for o, b in probes])


ONES = lambda n: [2] * n                    # n one-byte gap tokens (0x01): positions 1, 3, 5, ...
TAIL = ONES(40)


def _length(n):
    return designed(ONES(n), [(0, b"\x01" * n)])


def _boundary(B, k, j):
    D = D2 if k == 2 else D4
    assert len(gap(D)) == k and 0 < j < k
    return designed(ONES(B - j) + [D] + TAIL, [(0, b"\x01" * (B - j)), (B - j, gap(D)), (B - j + k, b"\x01" * 40)])


def _misleading(v, B, at):
    """the gap token of d - 1 = v placed so that its byte `at` - a continuation byte that reads like a token head - is stream byte B"""
    t = gap(v + 1)
    assert t[at] >= 0x80
    return designed(ONES(B - at) + [v + 1] + TAIL, [(B - at, t), (B, t[at:at + 1]), (B - at + len(t), b"\x01" * 40)])


def _run(n, B, behind):
    """a streak of n whose tokens end one byte before (behind = B - 1) or one byte after (B + 1) stream offset B"""
    nt = len(model([(2, n)])[1])
    items = ONES(behind - nt) + [(2, n)] + TAIL
    _, stream, first, end = model(items)
    assert end[behind - nt] == behind and nt >= 2
    return designed(items, [(behind - nt, stream[behind - nt:behind]), (behind, b"\x01" * 40)])


def _cell_crossing():
    items = ONES(500) + [(2, 70)] + TAIL
    pos = model(items)[0]
    assert 1023 in pos and 1024 in pos and pos[500] == 1001                 # (POS2_CELL = 1024 positions)
    return designed(items, [(500, b"\x01\xdf\xdf\xc4")])


def _streak_at_zero():
    return designed([(1, 40)] + TAIL, [(0, b"\x00\x00\xdf\xc5\x01")], comma=(100,))


def _n_longer_than_quality():
    n_at = list(range(1, 9001, 2))                                         # 4500 one-byte tokens: longer than a segment of either size
    c = designed(ONES(30), [(0, b"\x01" * 30)], n_at=n_at)
    c["npos"] = [b"\x01" * 4500]
    assert len(c["streams"][0][COLON]) < 4500
    return c


def _two_chunks():
    """chunk_bases 100,000: two chunks; ':' only in the first, ',' in both (its stream ends on a 4-byte gap's tail in the second), N only in the second"""
    n1 = 667 * READ                                                        # the first chunk: 667 reads (the first count that reaches 100,000 bases)
    colon = model(ONES(1100))[0]
    comma = [4, 8] + [n1 + p for p in model([D4] + ONES(20))[0]]
    return dict(fq=text({COLON: colon, COMMA: comma}, n_at=[n1 + p for p in model(ONES(1030))[0]], reads=MAX_READS), chunk_bases=100_000,
                streams=[{COLON: b"\x01" * 1100, COMMA: b"\x04\x03"}, {COLON: b"", COMMA: gap(D4) + b"\x01" * 20}], npos=[b"", b"\x01" * 1030], probes=[])


def _generated(nppm):
    fq1, _ = O.gen(O.NOVA_SE150, 1200, seed=5, nppm=nppm)
    return dict(fq=fq1, chunk_bases=1_000_000, streams=None, probes=[], want_n=nppm > 0)


BUILDERS = {}
for _n in (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097):
    BUILDERS["len_%d" % _n] = functools.partial(_length, _n)
for _B in EDGES:
    for _k in (2, 4):
        for _j in range(1, _k):
            BUILDERS["edge_%d_gap%d_minus%d" % (_B, _k, _j)] = functools.partial(_boundary, _B, _k, _j)
for _B in (16, 4096):                       # the first byte of a lane's 16; the first byte of a segment of any size
    for _v in (0x01C5, 0x01E3, 0x0185):
        BUILDERS["head_like_%04x_at_%d" % (_v, _B)] = functools.partial(_misleading, _v, _B, 1)
    for _at in (2, 3):
        BUILDERS["head_like_0001e3c5_byte%d_at_%d" % (_at, _B)] = functools.partial(_misleading, 0x0001E3C5, _B, _at)
for _B in EDGES:
    for _n in (33, 70):
        BUILDERS["run_%d_ends_before_%d" % (_n, _B)] = functools.partial(_run, _n, _B, _B - 1)
        BUILDERS["run_%d_ends_after_%d" % (_n, _B)] = functools.partial(_run, _n, _B, _B + 1)
BUILDERS["run_across_a_cell"] = _cell_crossing
BUILDERS["streak_at_position_0"] = _streak_at_zero
BUILDERS["n_many"] = functools.partial(_generated, 5000)
BUILDERS["n_none"] = functools.partial(_generated, 0)
BUILDERS["n_longer_than_quality"] = _n_longer_than_quality
BUILDERS["two_chunks_stream_absent"] = _two_chunks
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def image(name):
    """(case, its image): the streams the case designed ARE the image's, the bytes at the boundary it aims at are the intended ones - or the case fails here"""
    case = BUILDERS[name]()
    rfq = O.encode_file(case["fq"], b"", O.SE, case["chunk_bases"])
    h, chunks = S.parse(rfq)
    assert h.flags & S.H_QUAL_BY_COL and not h.flags & S.H_DONT_QUAL, h.flags
    got = [c.quality_streams()[0] for c in chunks]
    if case["streams"] is not None:
        assert len(chunks) == len(case["streams"]), (name, len(chunks))
        for g, want in zip(got, case["streams"]):
            for v, s in want.items():
                assert g[v] == s, (name, v, g[v][:64].hex(), s[:64].hex())
    for c, v, o, b in case["probes"]:
        assert got[c][v][o:o + len(b)] == b and len(b) > 0, (name, o, got[c][v][o:o + len(b)].hex(), b.hex())
    if "npos" in case:
        assert [c.npos for c in chunks] == case["npos"], name
    if "want_n" in case:                                                    # (a generated file: its N carry the N quality '#', whose stream codes them; many, or none at all)
        n_bases = sum(l.count(b"N") for l in case["fq"].split(b"\n")[1::4])
        assert (n_bases > 500 and len(got[0][ord("#")]) > 500) if case["want_n"] else (n_bases == 0 and not any(c.npos for c in chunks)), (name, n_bases)
    return case, rfq


def check(codec, name):
    """the image of case `name` decodes to its text under every segment size, on the fused path"""
    case, rfq = image(name)
    for seg in SEGS:
        codec.set_option("RFQ_POS_SEG", seg)
        got = codec.decode_bytes(rfq, split_pe=False)
        stages = dict(codec.timings())
        assert "emit" in stages and "emit_expanded" not in stages, (name, seg, sorted(stages))
        assert got == case["fq"], (name, seg, len(got), len(case["fq"]))


def write_fixtures(directory):
    """every case's image as NAME.rfq and its text as NAME.fq (tools/lists_asan.sh); -> the image paths"""
    out = []
    for name in NAMES:
        case, rfq = image(name)
        p = os.path.join(directory, name + ".rfq")
        with open(p, "wb") as f:
            f.write(rfq)
        with open(os.path.join(directory, name + ".fq"), "wb") as f:
            f.write(case["fq"])
        out.append(p)
    return out
