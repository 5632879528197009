"""Shared helpers of the N-bit tests (tests/test_emu_nbits.py on the SIMT interpreter, tests/test_gpu_nbits.py on the MI355X).

lnb, the "is N" bits of the loose slots k_gather2 leaves (a u16 per 16 bases), is all-zero between batches: the gather stores a word only where a base is N, its
readers - k_overlap<true>, k_seqpack - skip the slots of reads whose flag rn[] is clear, phase 2 of the gather zeroes the slots it packs again, and k_nbits_cleanup
zeroes what was set behind the last reader (rfq_ctx::lnb_dirty on the host).  A word that is not stored, not zeroed again or skipped where it holds a bit shows as
an N too many or too few - or an overlap found or missed - in some image, this call's or a later one's: every case here puts its N where one of those steps has an
edge, every image is compared whole with the oracle's (_oracle.encode_file, never the library), and the history circuit runs every input behind every other one on
ONE context.

Every case asserts that the tile path with match masks ran (stages `gather` and `quality_masks`): the byte-wise path has no loose slots."""
import collections
import random

import _engine as E
import _history as H
import _oracle as O
import _sections

CB = 20_000
Case = collections.namedtuple("Case", "name fq1 fq2 paired cb want")
_CASES = None
COMP = {65: 84, 84: 65, 67: 71, 71: 67, 78: 78}


def rc(s):
    return bytes(COMP.get(b, 78) for b in reversed(s))


def rand_seq(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def qual_of(i, seq):
    """'#' under an N, otherwise 'F' with a ':' now and then: three coded values - match masks"""
    return bytes(35 if c == 78 else (58 if (i + j) % 29 == 0 else 70) for j, c in enumerate(seq))


def record(i, seq, mate=1):
    return b"@A00250:26:H3YTWDSXX:1:1101:%d:%d %d:N:0:ACGT\n" % (1000 + i, 2000 + i // 7, mate) + bytes(seq) + b"\n+\n" + qual_of(i, seq) + b"\n"


def se_text(seqs):
    return b"".join(record(i, s) for i, s in enumerate(seqs))


def pe_texts(seqs1, seqs2):
    return b"".join(record(i, s) for i, s in enumerate(seqs1)), b"".join(record(i, s, 2) for i, s in enumerate(seqs2))


def chunk_reads(want):
    """reads per chunk of the oracle's image"""
    return [c.reads for c in _sections.parse(want)[1]]


def _seed_chunk0(seqs):
    """an N in chunk 0 (read 3): the header is made from chunk 0, and the N-position streams exist only where it has seen an N's quality"""
    seqs[3][len(seqs[3]) // 2] = 78


def _se150(n, seed):
    rng = random.Random(seed)
    seqs = [rand_seq(rng, 150) for _ in range(n)]
    _seed_chunk0(seqs)
    return seqs


def _bounds(seqs, cb):
    """[first read, end read) of every chunk - from the oracle's image of these reads (chunks are cut by bases, not by what the bases are)"""
    n = chunk_reads(O.encode_file(se_text(seqs), b"", O.SE, cb)); out = []; at = 0
    for k in n:
        out.append((at, at + k)); at += k
    assert at == len(seqs)
    return out


def _at_stored(seqs, first, pos):
    """(read, base) of stored position `pos` of the chunk that begins at read `first` (single-end: every base is stored)"""
    g = first
    while pos >= len(seqs[g]):
        pos -= len(seqs[g]); g += 1
    return g, pos


def _overlap_pairs(n, seed, special):
    """n pairs of 150 bases, every second one overlapping by 50 (RC(R2) begins with R1's last 50 bases: the header of such a file codes the mates by their overlap and
    k_seqpack trims RC(R2)'s first 50).  special(i, r1, rc2): edits of pair i before RC(R2) becomes R2 again."""
    rng = random.Random(seed); s1, s2 = [], []
    for i in range(n):
        r1 = rand_seq(rng, 150)
        rc2 = bytearray(r1[100:] + rand_seq(rng, 100)) if i % 2 == 0 else rand_seq(rng, 150)
        special(i, r1, rc2)
        s1.append(r1); s2.append(bytearray(rc(rc2)))
    s1[3][20] = 78                                                          # (chunk 0 holds an N: _seed_chunk0, outside every overlap)
    return s1, s2


def _coded_by_overlap(h, chunks):
    assert h.flags & _sections.H_PE_OVERLAP and all(c.flags & _sections.C_PE_INTERLEAVED for c in chunks), (hex(h.flags), [hex(c.flags) for c in chunks])


def cases():
    """{name: Case}, made once and never changed"""
    global _CASES
    if _CASES is not None:
        return _CASES
    made = collections.OrderedDict()

    def add(name, fq1, fq2=b"", paired=O.SE, cb=CB, min_chunks=2, check=None):
        want = O.encode_file(fq1, fq2, paired, cb)
        h, chunks = _sections.parse(want)
        assert h.flags & _sections.H_N_POS, name                              # (the N-position streams are there)
        assert len(chunks) >= min_chunks, (name, len(chunks))
        assert any(c.npos_size for c in chunks), name
        if check:
            check(h, chunks)
        made[name] = Case(name, fq1, fq2, paired, cb, want)

    # ---- an N as the first and as the last stored base of a chunk (chunk 2 of five)
    seqs = _se150(700, 101); b = _bounds(seqs, CB)
    assert len(b) >= 4
    seqs[b[2][0]][0] = 78; seqs[b[2][1] - 1][149] = 78
    add("chunk_first_and_last_base", se_text(seqs))
    # ---- a read of 150 bases ends inside a tight dword (150 = 9 * 16 + 6): the read behind it finishes that dword (take2).  An N in the last base of the one ...
    seqs = _se150(300, 102); seqs[150][149] = 78; seqs[40][149] = 78
    add("last_base_of_a_read_whose_dword_the_next_finishes", se_text(seqs))
    # ---- ... and in the first base of the other
    seqs = _se150(300, 103); seqs[151][0] = 78; seqs[41][0] = 78
    add("first_base_of_the_read_that_finishes_a_dword", se_text(seqs))
    # ---- reads of 1 to 15 bases in a row, N among them: a dword finished by many reads (the `while (filled < need)` loop), around read 256 of the chunk, where a
    # step of k_seqpack ends and the reads behind its SP_EXTRA = 8 LDS entries come from global memory
    rng = random.Random(104)
    seqs = [rand_seq(rng, 60) for _ in range(240)]
    _seed_chunk0(seqs)
    for i in range(60):
        seqs.append(bytearray(b"N" if i % 3 == 1 else bytes([rng.choice(b"ACGT")])))
    for rep in range(2):
        for ln in range(1, 16):
            s = rand_seq(rng, ln); s[(ln * 7 + rep) % ln] = 78
            seqs.append(s)
    seqs += [rand_seq(rng, 150) for _ in range(200)]
    seqs[340][5] = 78
    b = _bounds(seqs, CB)
    assert b[0][1] > 330, b                                                  # (all the short reads lie in chunk 0, on both sides of its read 256)
    add("reads_of_1_to_15_bases_in_a_row", se_text(seqs))
    # ---- overlapping mates, an N inside the part of RC(R2) that the overlap trims away (the overlap exists only if R1 holds the same N: a bit in R2's slot that
    # the tight stream never sees), and the same pair with the N in the first base behind the trimmed part
    for name, pos in (("n_inside_the_trimmed_overlap", 30), ("n_just_behind_the_trimmed_overlap", 50)):
        def special(i, r1, rc2, pos=pos):
            if i in (40, 170):
                assert i % 2 == 0
                rc2[pos] = 78
                if pos < 50:
                    r1[100 + pos] = 78
        s1, s2 = _overlap_pairs(260, 105, special)
        assert all(O.overlap(bytes(s1[i]), rc(s2[i])) == 50 for i in (40, 170))    # (the oracle's search takes R1 and RC(R2))
        a, b2 = pe_texts(s1, s2)
        add(name, a, b2, O.PE_TWO_FILES, check=_coded_by_overlap)
    # ---- a read of all N
    seqs = _se150(300, 107); seqs[160] = bytearray(b"N" * 150); seqs[161][:] = b"N" * 150; seqs[20][40:100] = b"N" * 60   # (chunk 0 holds fewer than 100 N: the reference codes N positions only then)
    add("a_read_of_all_n", se_text(seqs))
    # ---- a chunk without any N between two that hold some
    seqs = _se150(560, 108); b = _bounds(seqs, CB)
    assert len(b) >= 4
    for g in range(b[1][0], b[1][1], 9):
        seqs[g][(g * 31) % 150] = 78
    for g in range(b[3][0], b[3][1], 11):
        seqs[g][(g * 17) % 150] = 78

    def empty_between(h, chunks):
        assert chunks[1].npos_size > 8 and chunks[3].npos_size > 8 and chunks[2].npos_size < chunks[1].npos_size, [c.npos_size for c in chunks]
    add("a_chunk_without_n_between_two_with", se_text(seqs), check=empty_between)
    # ---- two files whose mates do not pair up in a chunk behind chunk 0: phase 2 of the gather repeats the chunk with R2 as it stands.  Phase 1 has packed R2 back
    # to front: an N at base 3 of 150 has left its bit at base 146 of the slot, which the repeat has to find zero
    rng = random.Random(109)
    s1 = [rand_seq(rng, 150) for _ in range(330)]; s2 = [rand_seq(rng, 150) for _ in range(330)]
    s1[3][20] = 78
    for g in (150, 151, 190):
        s2[g][3] = 78
    a, b2 = pe_texts(s1, s2)
    lines = b2.split(b"\n"); lines[4 * 160] = lines[4 * 160].replace(b":", b";", 1); b2 = b"\n".join(lines)

    def repeated(h, chunks):
        il = [bool(c.flags & _sections.C_PE_INTERLEAVED) for c in chunks]
        assert il[0] and not all(il), il
        at = 0
        for c, i in zip(chunks, il):                                         # (pairs 150, 151 and 190 lie in the chunk that is not interleaved)
            if not i:
                assert at <= 2 * 150 and 2 * 190 + 1 < at + c.reads, (at, c.reads)
            at += c.reads
    add("phase_2_repeats_a_chunk_with_n_in_r2", a, b2, O.PE_TWO_FILES, cb=30_000, check=repeated)
    # ---- one wave of k_overlap (64 consecutive pairs) with exactly one read that holds an N - an overlapping pair's in one case, another pair's in the other - between
    # waves without any; overlapping pairs in both kinds of wave
    for name, pair in (("one_n_in_a_wave_of_overlap_overlapping_pair", 64 + 20), ("one_n_in_a_wave_of_overlap_other_pair", 64 + 21)):
        def special(i, r1, rc2, pair=pair):
            if i == pair:
                rc2[120] = 78
        s1, s2 = _overlap_pairs(64 * 4, 110, special)
        assert O.overlap(bytes(s1[pair]), rc(s2[pair])) == (50 if pair % 2 == 0 else 0)
        assert sum(1 for s in s1 + s2 if 78 in s) == 2                        # (that read and chunk 0's, which is wave 0's: waves 2 and 3 hold none)
        a, b2 = pe_texts(s1, s2)
        add(name, a, b2, O.PE_TWO_FILES, check=_coded_by_overlap)
    _CASES = made
    return made


def check(codec, case):
    """the context's image of the case is the oracle's, and the tile path with match masks made it"""
    got = E.encode(codec, case.fq1, case.fq2, case.paired, case.cb)
    marks = {n for n, _ in codec.timings()}
    assert "gather" in marks and "quality_masks" in marks, (case.name, sorted(marks))
    msg = H.image_diff(got, case.want)
    assert not msg, (case.name, msg)


# ---------------------------------------------------------------- history: every input behind every other one on one context
# marks: stage names the call must (with "!": must not) show
Step = collections.namedtuple("Step", "name fq1 fq2 paired cb want opts marks")
_STEPS = None


def history_inputs():
    """(a) N-rich PE150; (b) the same records without any N; (c) N-rich reads of another length (100): slots and chunk bases shift, a bit left behind lands in another
    read; (d) an input on the byte-wise path, which leaves the loose slots alone; (e) an N-rich input with four equally frequent quality values - the arenas sized in advance
    are too small for it wherever the context has not grown them: the batch is repeated inside the call"""
    global _STEPS
    if _STEPS is not None:
        return _STEPS
    made = []

    def add(name, fq1, fq2, paired, cb, opts=None, marks=("gather", "quality_masks")):
        made.append(Step(name, fq1, fq2, paired, cb, O.encode_file(fq1, fq2, paired, cb), dict(opts or {}), tuple(marks)))
    # (N at 2000 ppm: one read in three holds one - and chunk 0 fewer than 100, so the header codes N positions)
    a, b = O.gen(O.NOVA_PE150, 400, seed=71, nppm=2000)
    assert sum(1 for s in a.split(b"\n")[1::4] + b.split(b"\n")[1::4] if b"N" in s) > 200
    add("a_pe150_n_rich", a, b, O.PE_TWO_FILES, CB)
    assert _sections.parse(made[-1].want)[0].flags & _sections.H_N_POS

    def without_n(fq):
        ln = fq.split(b"\n")
        for i in range(1, len(ln), 4):
            ln[i] = ln[i].replace(b"N", b"A")
        return b"\n".join(ln)
    a0, b0 = without_n(a), without_n(b)
    assert (a0, b0) != (a, b) and len(a0) == len(a)
    seq_lines = b"".join(a0.split(b"\n")[1::4]) + b"".join(b0.split(b"\n")[1::4])
    assert b"N" not in seq_lines
    add("b_pe150_no_n", a0, b0, O.PE_TWO_FILES, CB)
    rng = random.Random(72); s1 = [rand_seq(rng, 100) for _ in range(500)]; s2 = [rand_seq(rng, 100) for _ in range(500)]
    for i, s in enumerate(s1 + s2):
        if i % 3 == 0:
            s[rng.randrange(100)] = 78
    a, b = pe_texts(s1, s2)
    add("c_pe100_n_rich", a, b, O.PE_TWO_FILES, CB)
    a, _ = O.gen(O.NOVA_SE150, 600, seed=73, nppm=3000)
    add("d_byte_wise_path", a, b"", O.SE, CB, opts={"RFQ_GATHER": "old"}, marks=("gather_bytes", "!gather"))
    rng = random.Random(74); recs = []
    for i in range(900):
        seq = rand_seq(rng, 150)
        if i % 4 == 0:
            seq[rng.randrange(150)] = 78
        q = bytes(rng.choice(b"F:,5") for _ in range(150))
        recs.append(b"@M:1:FC:1:%d:%d:%d 1:N:0:AC\n" % (1101 + i // 500, rng.randrange(1000, 30000), rng.randrange(1000, 60000)) + bytes(seq) + b"\n+\n" + q + b"\n")
    add("e_arenas_too_small", b"".join(recs), b"", O.SE, 30_000)
    _STEPS = made
    return made


def history_step(codec, st):
    """'' or what is wrong with the context's image (or the stages) of the input"""
    with E.Options(codec, st.opts):
        got = E.encode(codec, st.fq1, st.fq2, st.paired, st.cb)
        marks = {n for n, _ in codec.timings()}
    if not H.marks_ok(marks, st.marks):
        return "stages %s, expected %s" % (sorted(marks), st.marks)
    return H.image_diff(got, st.want)


def check_history(make_codec):
    """every ordered pair of the five inputs adjacent once, on one context; the first call of the circuit is (e)'s on the fresh context: its arenas are too small and
    the batch is repeated inside the call (stage `retry_room`)"""
    steps = history_inputs(); k = len(steps)
    seq = H.euler(k)
    e = k - 1
    seq = [(i + e) % k for i in seq]                                          # (a relabelled circuit is a circuit: it starts at (e))
    assert seq[0] == e and sorted(set(zip(seq, seq[1:]))) == [(x, y) for x in range(k) for y in range(k)]
    codec = make_codec(); bad = []; prev = "a fresh context"
    for n, i in enumerate(seq):
        st = steps[i]
        msg = history_step(codec, st)
        if n == 0:
            marks = {s for s, _ in codec.timings()}
            assert "retry_room" in marks, sorted(marks)
        if msg:
            bad.append("step %d: %s behind %s: %s" % (n, st.name, prev, msg))
        prev = st.name
    assert not bad, "%d of %d steps differ from the oracle:\n%s" % (len(bad), len(seq), "\n".join(bad[:12]))
