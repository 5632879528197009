"""Two-file PE through one line index, match-mask form (k_gather2<true, 1, true>): the proof that R2's lines are where R1's table says sits in the lanes that hold
the bytes - base line: the exact path behind pack16_fast; quality line: the `rest` loop, and a guard on the header's major / dense values; name and '+' line: the
read's lanes over the lines' 16-byte groups; the four line ends as before.  Fixtures, inputs and helpers are tests/test_mirror_index.py's: -k 100, 700 NovaSeq pairs
(chunks of 334 pairs; tiles of 64 reads or, with a workgroup per tile, of 62), a fresh `on` context per case, compared with the RFQ_MIRROR=0 context and the oracle.
A case that must fall back asserts the `mirror_fallback` marker and equality with the `off` context's result or error: it never passes as "mirrored and happened to
be equal".  Two kinds of result carry no marker of their own call and are named in must_fall_back: the error found on the normalised text (a '\r' or a line feed
inside a quality line: "a quality line is shorter ...") and the empty result (a line feed in the place of record 0's '+') collect no stage times; there the equality
is asserted alone.  Where the result is another error (a base the reference refuses in chunk 0) the marker is collected and asserted, but the repeat is encode_impl's
doing whatever the gather said: the gather's own verdict is tested by the cases behind chunk 0, which is where most of the sampled records lie."""
import itertools
import random

import pytest

import _oracle as O
from test_mirror_index import CB, check_fallback, fell_back, make, mirrored, nl_pos, off, on, pe, records, run, text   # noqa: F401  (make, off, on: fixtures)

CTL = [0x00, 0x09, 0x0A, 0x0D, 0x0F]
# (line of the record, byte of the line; negative: from the line's end).  Names of the generated files are shorter than 64 bytes: "name_long" first gives the record
# a name of 100 bytes in both files.
POSITIONS = [("base", 0), ("base", 72), ("base", 143), ("base", 144), ("base", 149),
             ("qual", 0), ("qual", 72), ("qual", 143), ("qual", 144), ("qual", 149),
             ("name", 0), ("name", 20), ("name_long", 70), ("name", -1), ("plus", 0)]
# pair 0 of chunk 0 and its last pair; in chunk 1 (pairs 334 .. 667, where the verdict is the gather's own): its first pair, the last read of a tile and the first of the
# next (62 or 64 reads: pairs 364 | 365 | 366), which is also where a workgroup's share ends (395: the second share's last pair), its last pair; the first pair of
# chunk 2 and the last encoded pair
PAIRS_HIT = [0, 333, 334, 364, 365, 366, 395, 667, 668, 699]
LINE = {"name": 0, "name_long": 0, "base": 1, "plus": 2, "qual": 3}


def _grid():
    full = list(itertools.product(POSITIONS, PAIRS_HIT, CTL))
    picked = random.Random(13).sample(full, 60)
    for p in POSITIONS:                                      # every position, record and value at least once
        assert any(c[0] == p for c in picked)
    assert {c[1] for c in picked} == set(PAIRS_HIT) and {c[2] for c in picked} == set(CTL)
    return picked


def _oracle(a, b):
    """the oracle's image, or None where it refuses the text as the reference does (a base that is no upper-case letter)"""
    try:
        return O.encode_file(a, b, O.PE_TWO_FILES, CB)
    except O.OracleError:
        return None


def no_markers(res):
    """results whose call collects no stage times: the empty result, and the error that the attempt on the normalised text returns"""
    return (res[0] == 0 and not res[2]) or (res[0] < 0 and "a quality line is shorter than its sequence line" in res[1])


def must_fall_back(on, off, a, b, want=None):
    ref, m0 = run(off, a, b)
    got, m = run(on, a, b)
    assert got == ref, (got[:2], ref[:2], got[3:], ref[3:])
    if not no_markers(ref):
        assert fell_back(m), (ref[:2], sorted(m))
    if ref[0] == 0 and ref[2] and want is not None:
        assert got[:3] == (0, "", want) and got[3:5] == (len(a), len(b))
    return got


def _put(line, i, v):
    b = bytearray(line); b[i] = v
    return bytes(b)


def _lengthen(r1, r2, k, n):
    """record k gets a name of n bytes in both files: the mates stay aligned"""
    for r in (r1, r2):
        r[k][0] += b" " + b"x" * (n - len(r[k][0]) - 1)
        assert len(r[k][0]) == n


@pytest.mark.parametrize("pos,k,v", _grid(), ids=lambda x: "%s%d" % x if isinstance(x, tuple) else "%d" % x)
def test_one_control_byte_in_r2_falls_back(on, off, pos, k, v):
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2)
    assert len(r2) == 700 and len(r2[k][1]) == 150
    if pos[0] == "name_long":
        _lengthen(r1, r2, k, 100)
    a = text(r1)
    r2[k][LINE[pos[0]]] = _put(r2[k][LINE[pos[0]]], pos[1], v)
    bad = text(r2)
    assert len(bad) == len(a)
    # (a line feed or a carriage return changes what the text is; any other value is a letter like the rest: the oracle has an answer)
    must_fall_back(on, off, a, bad, want=_oracle(a, bad) if v not in (0x0A, 0x0D) else None)


@pytest.mark.parametrize("pos", POSITIONS, ids=lambda p: "%s%d" % p)
def test_every_position_in_a_later_chunk(on, off, pos):
    """the same at every position of a record of chunk 1, with values that leave the text a FASTQ file: chunk 0 alone makes the header (and is where the reference
    looks at the letters of the bases), so the result is an image and the verdict is the gather's own"""
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2); k = 401
    if pos[0] == "name_long":
        _lengthen(r1, r2, k, 100)
    a = text(r1)
    r2[k][LINE[pos[0]]] = _put(r2[k][LINE[pos[0]]], pos[1], (0x00, 0x09, 0x0F)[POSITIONS.index(pos) % 3])
    bad = text(r2)
    got = must_fall_back(on, off, a, bad, want=_oracle(a, bad))
    assert got[0] == 0 and got[2] or pos == ("name", 0)             # (a record without its '@' may be refused)


@pytest.mark.parametrize("line", ["base", "qual"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32])
def test_short_reads_with_a_carriage_return(on, off, n, line):
    """reads of n bases in both files (one group, a group and a moved-back one, two whole groups), a '\\r' in the place of the last base / quality of an R2 read - and a
    0x0F, which leaves the text a FASTQ file.  Where n allows it the records are repeated until they fill more than one chunk and the byte sits in the last pair:
    behind chunk 0 the result is an image, and the verdict the gather's own."""
    fq1, fq2, _ = pe()
    mult = 1 if n == 1 else -(-200_000 // (1400 * n))              # (two chunks of 100,000 bases and more)
    r1, r2 = ([list(rec) for _ in range(mult) for rec in records(f)] for f in (fq1, fq2))
    for r in (r1, r2):
        for rec in r:
            rec[1] = rec[1][:n]; rec[3] = rec[3][:n]
    a, b = text(r1), text(r2)
    got, m = run(on, a, b)
    assert mirrored(m) and got[:3] == (0, "", O.encode_file(a, b, O.PE_TWO_FILES, CB))
    k = len(r2) - 1; good = r2[k][LINE[line]]
    for v in (0x0D, 0x0F):
        r2[k][LINE[line]] = _put(good, n - 1, v)
        got = must_fall_back(on, off, a, text(r2))
        assert v == 0x0D or n == 1 or (got[0] == 0 and got[2])


@pytest.mark.parametrize("line", ["name_100", "name_300", "name_300_read0", "plus_repeats_name"])
def test_control_byte_ends_a_long_line(on, off, line):
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2)
    k = 0 if line == "name_300_read0" else 380
    if line == "plus_repeats_name":
        for r in (r1, r2):
            r[k][2] = b"+" + r[k][0][1:]
    else:
        _lengthen(r1, r2, k, 100 if line == "name_100" else 300)
    a, b = text(r1), text(r2)
    got, m = run(on, a, b)
    assert mirrored(m) and got[:3] == (0, "", O.encode_file(a, b, O.PE_TWO_FILES, CB))
    li = 2 if line == "plus_repeats_name" else 0
    r2[k][li] = _put(r2[k][li], -1, 0x09)
    bad = text(r2)
    must_fall_back(on, off, a, bad, want=_oracle(a, bad))


def test_control_value_known_to_the_header(on, off):
    """0x0B in the place of R2's most frequent quality throughout chunk 0 (and ',' folded into ':' so that the file keeps its match-mask form): a value below 0x10 is a
    dense one, no lane ever takes it out of its group - the kernel refuses the table at its start"""
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2)
    for r in (r1, r2):
        for rec in r:
            rec[3] = rec[3].replace(b",", b":")
    top = max(set(b"".join(rec[3] for rec in r2[:334])), key=b"".join(rec[3] for rec in r2[:334]).count)
    for rec in r2[:334]:
        rec[3] = rec[3].replace(bytes([top]), b"\x0b")
    a, b = text(r1), text(r2)
    assert nl_pos(a) == nl_pos(b)
    _, m0 = run(off, a, b)
    assert "quality_masks" in m0, sorted(m0)
    must_fall_back(on, off, a, b, want=_oracle(a, b))


@pytest.mark.parametrize("what", ["bases_N", "bases_lower_case_and_dot", "quals_outside_the_table"])
def test_rare_paths_without_a_control_byte_stay_mirrored(on, off, what):
    """the exact path of the base packer and the `rest` loop of the qualities, taken for bytes that are no control bytes: no false alarm.  (Lower-case bases and '.'
    behind chunk 0: the reference looks at the letters in chunk 0 only - there it refuses the file, test_bases_the_reference_refuses.)"""
    fq1, fq2, _ = pe()
    r2 = records(fq2)
    if what == "bases_N":
        for k, i in {0: 0, 31: 75, 332: 144, 333: 149, 500: 16, 699: 148}.items():
            r2[k][1] = _put(r2[k][1], i, ord("N"))
    elif what == "bases_lower_case_and_dot":
        for k, (i, c) in {334: (0, b"a"), 365: (75, b"."), 401: (144, b"n"), 500: (149, b"t"), 667: (16, b"."), 668: (143, b"c"), 699: (148, b"g")}.items():
            r2[k][1] = _put(r2[k][1], i, c[0])
    else:
        for k, (i, c) in {340: (0, b"Z"), 400: (149, b"!"), 699: (144, b"\x7f"), 698: (15, b"\x10")}.items():     # (chunk 0 makes the table)
            r2[k][3] = _put(r2[k][3], i, c[0])
    b = text(r2)
    got, m = run(on, fq1, b)
    assert mirrored(m), sorted(m)
    assert got[:5] == (0, "", O.encode_file(fq1, b, O.PE_TWO_FILES, CB), len(fq1), len(b)) and got == run(off, fq1, b)[0]


@pytest.mark.parametrize("c", [b"a", b"n", b"."])
def test_bases_the_reference_refuses(on, off, c):
    """a lower-case base or a '.' in chunk 0 of R2: the reference refuses the file when it makes the header, and the error is the other context's (an error of an
    attempt through one table is always repeated with both)"""
    fq1, fq2, _ = pe()
    r2 = records(fq2); r2[31][1] = _put(r2[31][1], 75, c[0]); r2[699][1] = _put(r2[699][1], 148, c[0])
    b = text(r2)
    assert _oracle(fq1, b) is None
    got, m = run(on, fq1, b)
    assert got[0] < 0 and got == run(off, fq1, b)[0]


@pytest.mark.parametrize("v", [0x10, 0x1F, 0x80, 0xFF])
def test_other_odd_bytes_in_a_name(on, off, v):
    """not control bytes in the test's sense (0x10 right behind one would be): the result is the other context's, by either path"""
    fq1, fq2, _ = pe()
    r2 = records(fq2)
    for k, i in ((0, 5), (380, 30), (699, -1)):
        r2[k][0] = _put(r2[k][0], i, v)
    b = text(r2)
    got, m = run(on, fq1, b)
    assert mirrored(m) or fell_back(m), sorted(m)
    assert got == run(off, fq1, b)[0]


def test_unterminated_last_record_ends_in_a_control_byte(on, off):
    fq1, fq2, _ = pe()
    a, b = fq1[:-1], fq2[:-2] + b"\t"
    assert len(a) == len(b)
    must_fall_back(on, off, a, b, want=_oracle(a, b))


def test_byte_stream_form_still_counts(on, off):
    """BGI_PE100 with forty quality values: k_gather2<false> - a line feed moved inside a record falls back through the count"""
    fq1, fq2, _ = pe(O.BGI_PE100)
    ends = nl_pos(fq2)[0:4]
    b = bytearray(fq2); b[ends[1]] = ord("A"); b[ends[2] + 40] = 10
    got, m = run(on, fq1, fq2)
    assert mirrored(m) and "quality_masks" not in m
    check_fallback(on, off, fq1, bytes(b))


def _unpair(r2):
    """R2's names end in another letter than R1's: the mates differ in two places, the header does not support interleaving and phase 1 takes R2 as it stands"""
    for rec in r2:
        rec[0] = rec[0][:-1] + (b"Z" if rec[0][-1:] != b"Z" else b"Y")


@pytest.mark.parametrize("i", [0, 72, 144, 149])
def test_control_byte_in_bases_of_mates_that_do_not_pair(on, off, i):
    """the forward orientation of the base packer's exact path"""
    fq1, fq2, _ = pe()
    r2 = records(fq2); _unpair(r2)
    b = text(r2)
    assert nl_pos(b) == nl_pos(fq1)
    got, m = run(on, fq1, b)
    assert mirrored(m) and got[:3] == (0, "", O.encode_file(fq1, b, O.PE_TWO_FILES, CB))
    r2[401][1] = _put(r2[401][1], i, 0x0F)
    bad = text(r2)
    got = must_fall_back(on, off, fq1, bad, want=_oracle(fq1, bad))
    assert got[0] == 0 and got[2]


def test_control_byte_behind_a_short_sequence_line(on, off):
    """record 401 of both files has a sequence line of 149 bases and a quality line of 150 bytes: the quality lanes look at 149, the control byte is the 150th"""
    fq1, fq2, _ = pe()
    r1, r2 = records(fq1), records(fq2)
    for r in (r1, r2):
        r[401][1] = r[401][1][:-1]; r[401][0] += b"x"
    a = text(r1)
    r2[401][3] = _put(r2[401][3], 149, 0x0F)
    bad = text(r2)
    assert len(a) == len(bad)
    must_fall_back(on, off, a, bad, want=_oracle(a, bad))
