"""Shared helpers of the history tests (tests/test_emu_history.py on the SIMT interpreter, tests/test_gpu_history.py on the MI355X): what a context carries
from one call to the next (rfq_ctx: rec_per_byte / lazy_block, mixed_lengths, dense_ok, e3_pieces_failed, mirror_block, the qplane_* bookkeeping, 120 buffers that
only grow, the context-owned results of the rows family) is pinned by running every input behind every other one on ONE context.

The order is an Eulerian circuit of the complete digraph with loops (euler): k * k + 1 calls see each of the k * k ordered pairs (predecessor, input) once.  The
expected results never come from the library: _oracle.encode_file gives the image, _oracle.decode_file of that image the text, both computed once (inputs()).

Refusals are part of a context's history too: the encoder and the decoder leave by many exits, each with state behind it (buffers marked dirty, a header made from
the refused text, read-backs pending into a frame that has returned, a forked stream to join).  refusals() makes one refusing input per exit, each proven against the
oracle, and refusal_circuit() walks every ordered pair over the good and the refusing inputs that the circuits above do not have (circuit, refusal_edges).  The same
over the kinds of call (calls_refusal_circuit), and a small batch behind a large one for every rows call whose scratch only grows (check_nothing_left)."""
import collections
import functools
import threading

import numpy as np

import _engine as E
import _oracle as O
import _sections


def circuit(nodes, edges):
    """a closed walk over `nodes` that uses every (a, b) of `edges` exactly once (Hierholzer; the digraph must be connected, every node with as many edges in as out -
    a walk that does not close or leaves an edge out fails here)"""
    nodes, edges = list(nodes), list(edges)
    left = {a: [] for a in nodes}                                            # the edges a -> b not walked yet
    for a, b in edges:
        left[a].append(b)
    stack, out = [nodes[0]], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == len(edges) + 1 and out[0] == out[-1], (len(nodes), len(edges), len(out))
    assert collections.Counter(zip(out, out[1:])) == collections.Counter(edges) and len(set(edges)) == len(edges), (len(nodes), len(edges))
    return out


def euler(k):
    """k * k + 1 indices in which every ordered pair (a, b) of range(k), a == b included, is adjacent exactly once: the complete digraph with loops"""
    out = circuit(range(k), [(a, b) for a in range(k) for b in range(k)])
    assert len(out) == k * k + 1, (k, len(out))
    return out


def refusal_edges(g, r):
    """nodes 0 .. g - 1 are good, g .. g + r - 1 refuse: every ordered pair but good -> good (those are euler(g)'s) - 2 * g * r + r * r edges, refusal behind refusal
    and a refusal behind itself among them; every node has g + r edges in and out but the good ones, which have r and r"""
    return [(a, b) for a in range(g + r) for b in range(g + r) if a >= g or b >= g]


# ---------------------------------------------------------------- the inputs
# want: the oracle's image; text: the oracle's decode of it (a pair of texts where `split`); caller: the decode goes into caller buffers (the emitter is launched ahead
# of the host's look at the status); state: the context state the input is there for; enc_mark / dec_mark: stage names of codec.timings() a FRESH context must (with
# "!": must not) show on its first encode / decode of it; enc2_mark: the same for a second encode on that context (`lazy_index`: the index without a read-back, which the
# context can do once it knows the records per byte and which a text that has to be normalised or ends at an empty line never gets).  What no stage name shows is
# asserted on the oracle's image instead (add(check=...)): the chunk flags, the header's table.
Input = collections.namedtuple("Input", "name fq1 fq2 paired cb want text split caller state enc_mark dec_mark enc2_mark")
_INPUTS = None


def _text(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def _records(fq):
    ln = fq.split(b"\n")
    assert ln[-1] == b""
    return [ln[i:i + 4] for i in range(0, len(ln) - 1, 4)]


def _qual_recs(n, quals, seed):
    """n SE150 records whose quality bytes are drawn evenly from `quals` (the text of _engine.check_every_repeat_in_one_call)"""
    import random
    rng = random.Random(seed)

    def rec(i):
        seq = bytes(rng.choice(b"ACGT") for _ in range(150)); q = bytes(rng.choice(quals) for _ in range(150))
        return b"@M:1:FC:1:%d:%d:%d 1:N:0:AC\n" % (1101 + i // 500, rng.randrange(1000, 30000), rng.randrange(1000, 60000)) + seq + b"\n+\n" + q + b"\n"
    return b"".join(rec(i) for i in range(n))


def _rare_recs(n, seed):
    """n SE150 records: quality 'F' but for about 1 byte in 400, drawn from ':', ',' and '5'; from record 200 on (chunk 0 ends before it at 20,000 bases a chunk)
    one byte in 1500 is '<', which the header's table - made from chunk 0 - does not hold: an exception"""
    import random
    rng = random.Random(seed); out = []
    for i in range(n):
        seq = bytes(rng.choice(b"ACGT") for _ in range(150)); q = bytearray(b"F" * 150)
        for j in range(150):
            if rng.random() < 1 / 400:
                q[j] = rng.choice(b":,5")
            if i >= 200 and rng.random() < 1 / 1500:
                q[j] = ord("<")
        out.append(b"@M:1:FC:1:%d:%d:%d 1:N:0:AC\n" % (1101 + i // 500, rng.randrange(1000, 30000), rng.randrange(1000, 60000)) + seq + b"\n+\n" + bytes(q) + b"\n")
    return b"".join(out)


def _rare_planes_are_reached(fq1, want):
    """Match-mask mode takes files of up to four coded values and keeps at most THREE dense planes (rfq_encode.hip: M.nd = min(n_normal, 3), two where the tile has no
    room for three - reads of 150 bases); the other coded values and every byte outside the header's table (the exception plane) are set bit by bit in RARE planes,
    listed in rare[] and zeroed again by k_rare_cleanup.  This text has four coded values - three that occur in every chunk and the 0xFF entry the reference appends
    for a file without N bases - and, in every chunk behind the first, bytes outside the table: bits in the exception plane whatever the dense planes are, and in a
    coded value's plane where there are two.  Few enough per chunk that rare[] stays a list (<= G2_RARE_LIST = 255 words): the cleanup's sparse branch - its other
    branch, the whole extent, is four_quals' (a quarter of all bytes in the fourth plane)."""
    h, chunks = _sections.parse(want)
    assert sorted(h.normal) == sorted(b":,5\xff") and len(chunks) >= 3, (h.normal, len(chunks))
    quals = [r[3] for r in _records(fq1)]; at = 0
    for k, c in enumerate(chunks):
        q = b"".join(quals[at:at + c.reads]); at += c.reads
        counts = [q.count(bytes([v])) for v in b":,5"]; exc = q.count(b"<")
        assert min(counts) >= 1 and (exc >= 1) == (k > 0) and sum(counts) + exc <= 255, (k, counts, exc)
    assert at == len(quals)


def _chunk_flags(test):
    """a check for add(): `test(flags, reads)` holds for every chunk of the oracle's image"""
    def check(fq1, want):
        _, chunks = _sections.parse(want)
        assert chunks and all(test(c.flags, c.reads) for c in chunks), [(hex(c.flags), c.reads) for c in chunks]
    return check


def inputs():
    """the thirteen texts, made once and never changed"""
    global _INPUTS
    if _INPUTS is not None:
        return _INPUTS
    made = []

    def add(name, fq1, fq2, paired, cb, state, enc_mark=(), dec_mark=(), enc2_mark=(), caller=False, lossless=True, check=None):
        want = O.encode_file(fq1, fq2, paired, cb)
        if check:
            check(fq1, want)
        split = paired == O.PE_TWO_FILES
        text = O.decode_file(want, split)
        if lossless:
            assert text == ((fq1, fq2) if split else fq1), name
        size, chunks = len(fq1) + len(fq2), len(O.chunk_table(want)) - 1
        if name != "three_records":
            assert 100_000 <= size <= 350_000 and 2 <= chunks <= 6 and 10_000 <= cb <= 30_000, (name, size, chunks, cb)
        made.append(Input(name, fq1, fq2, paired, cb, want, text, split, caller, state, tuple(enc_mark), tuple(dec_mark), tuple(enc2_mark)))

    a, b = O.gen(O.NOVA_PE150, 400, seed=11)
    add("pe150", a, b, O.PE_TWO_FILES, 30000, "mirrored index", enc_mark=("mirror_index", "!mirror_fallback"), enc2_mark=("mirror_index", "lazy_index"))
    # (tests/test_mirror_index.py::test_names_of_other_lengths_fall_back: one name of R2 a byte longer, the next a byte shorter - sizes equal, two line ends moved)
    a, b = O.gen(O.NOVA_PE150, 330, seed=19)
    r2 = _records(b); r2[170][0] += b"A"; r2[171][0] = r2[171][0][:-1]; b = _text(r2)
    assert len(a) == len(b)
    add("pe_unmirrored", a, b, O.PE_TWO_FILES, 30000, "mirror_block", enc_mark=("mirror_fallback", "!mirror_index"))
    a, _ = O.gen(O.SE_VAR, 500, seed=13)
    add("se_var", a, b"", O.SE, 15000, "mixed_lengths", check=_chunk_flags(lambda fl, n: not fl & _sections.C_READ_LEN_SAME))
    a, b = O.gen(O.BGI_PE100, 450, seed=14, n_quals=40)
    add("bgi_q40", a, b, O.PE_TWO_FILES, 20000, "no match masks (dense_ok stays down)", enc_mark=("!quality_masks",))
    add("four_quals", _qual_recs(900, b"F:,5", 5), b"", O.SE, 30000, "arenas sized too small: the room repeat", enc_mark=("retry_room", "quality_masks"))
    a = _rare_recs(600, 6)
    add("rare_quals", a, b"", O.SE, 20000, "rare planes: exceptions and a coded value beyond the dense ones, a short rare[] list per chunk (k_rare_cleanup)",
        enc_mark=("quality_masks",), check=_rare_planes_are_reached)
    # (the `mixed` text of _engine.check_pieces_remembered_behind_speculative_emit, with 60 long names for its 80: that test has ONE chunk of 900 reads, here a chunk
    # is 300 reads, and plan_fused sizes the name tile by the chunk's AVERAGE name - 80 names of 114 bytes among 300 average 41 bytes, which selects the 13 KB tile
    # that holds 64 of them: no retry, no state.  60 average 35 bytes: the 3 KB tile, which a run of 27 long names overflows)
    a = E.handmade(900, lambda i: ("SRR0123456.%d" % i) if not 400 <= i < 460 else ("L" * 110 + "%d" % i), lambda i: 100, lambda i: "+", seed=4,
                   qual_of=lambda i, j: "F" if (i + j) % 29 else ",")
    add("long_names", a, b"", O.SE, 30000, "e3_pieces_failed", dec_mark=("emit", "emit_expanded"), caller=True)
    a, _ = O.gen(O.SE_VAR, 400, seed=17)
    add("crlf", a.replace(b"\n", b"\r\n"), b"", O.SE, 15000, "the normalising path", lossless=False, enc2_mark=("!lazy_index",))
    a = _qual_recs(500, b"FFFFFF:,", 7)
    add("empty_line", a + b"\n" + _qual_recs(3, b"FFFFFF:,", 8), b"", O.SE, 20000, "the repeat that ends the input at an empty line", lossless=False, enc2_mark=("!lazy_index",))
    a, _ = O.gen(O.NOVA_PE150, 250, seed=18, interleaved=True)
    add("interleaved", a, b"", O.PE_INTERLEAVED, 20000, "pairs in one text", enc2_mark=("lazy_index",), check=_chunk_flags(lambda fl, n: fl & _sections.C_PE_INTERLEAVED))
    a, _ = O.gen(O.NOVA_SE150, 970, seed=15)
    add("se150_big", a, b"", O.SE, 30000, "the buffers grow (rec_per_byte of a uniform file)", enc2_mark=("lazy_index",),
        check=_chunk_flags(lambda fl, n: fl & _sections.C_READ_LEN_SAME))
    a, _ = O.gen(O.NOVA_SE150, 3, seed=16)
    add("three_records", a, b"", O.SE, 30000, "buffers far larger than the batch", enc2_mark=("lazy_index",), check=_chunk_flags(lambda fl, n: n == 3))
    # (a lower-case base is refused where the header is made - chunk 0, RfqHeader::makeQualityTable - and nowhere else: behind it the reference encodes the byte as it
    # does any base that is not A/C/G/T.  The thirteenth input pins that image; the same byte in chunk 0 is refusals()' lowercase_chunk0)
    recs = _records(by_name_in(made, "four_quals").fq1); seq = bytearray(recs[-5][1]); seq[70] = ord("a"); recs[-5][1] = bytes(seq)
    add("lowercase_late", _text(recs), b"", O.SE, 30000, "a byte outside A/C/G/T/N behind chunk 0, under match masks", enc_mark=("quality_masks",), lossless=False)
    assert max(len(i.fq1) + len(i.fq2) for i in made) == len(made[10].fq1) and made[10].name == "se150_big"
    _INPUTS = made
    return made


def by_name_in(made, name):
    return next(i for i in made if i.name == name)


def by_name(name):
    return by_name_in(inputs(), name)


# ---------------------------------------------------------------- the refusing inputs
# Every one is a good text (image) with ONE mutation; refusals() proves on the CPU that the oracle takes the one and refuses the other.  What a step must raise:
# codes - the RFQ_E_* values allowed (include/rfq_hip.h: RFQ_E_DATA "the reference would error_exit on this input (message = its text)", RFQ_E_UNPINNED for the two
# inputs both sides refuse rather than reproduce, RFQ_E_NOSPACE for a caller's buffer); message - the oracle's text, compared by the rule of _engine.check_case /
# _fuzz.check (equal but for surrounding white space), or phrase - the key phrase of a refusal both sides word in their own way (_fuzz.check_block); neither for a
# refusal that is pinned by its code alone.  kind "enc": fq1 / fq2 / paired / cb, short - the caller's d_out holds that many bytes; kind "dec": image / split / caps /
# chunk_off.  text - what the library must RETURN, for the one hostile input that is no refusal (an image with a chunk index that lies: the index is not verified and
# the chain is walked, include/rfq_hip.h, rfq_decode_args.h_chunk_off - the oracle knows no index and decodes the image).
RFQ_E_DATA, RFQ_E_UNPINNED, RFQ_E_NOSPACE = -5, -7, -8
Refusal = collections.namedtuple("Refusal", "name kind src exit codes message phrase fq1 fq2 paired cb short image split caps chunk_off text")
_REFUSALS = None
MUTANT_LABELS = {}                                                           # {name: (history image, the label _hostile.mutants gave the mutant)}
QUAL_OVERFLOW_SEED = 12
COORD_MAX = 2097152                                                          # (RfqCodec::encodeCoords refuses what is LARGER than 2M - 1: this value is the first)


def _refusal(name, kind, src, exit, codes, message=None, phrase=None, fq1=b"", fq2=b"", paired=0, cb=0, short=None, image=b"", split=False, caps=None, chunk_off=None,
             text=None):
    return Refusal(name, kind, src, exit, tuple(codes), message, phrase, fq1, fq2, paired, cb, short, image, split, caps, chunk_off, text)


def _oracle_refuses(fq1, fq2, paired, cb):
    try:
        O.encode_file(fq1, fq2, paired, cb)
    except O.OracleError as e:
        return str(e)
    return None


def _with_coord(name_line, axis, value):
    """an Illumina name line (@instrument:run:flowcell:lane:tile:x:y[ comment]) with its x (axis 5) or y (axis 6) replaced"""
    head, sep, comment = name_line.partition(b" ")
    f = head.split(b":")
    assert len(f) == 7, name_line
    f[axis] = b"%d" % value
    return b":".join(f) + sep + comment


def _late(fq1, fq2, paired, cb, rec):
    """the oracle's image of the text cut in front of record `rec` (of each file) has at least two chunks: the mutation is behind chunk 0 and behind another chunk"""
    a = _text(_records(fq1)[:rec]); b = _text(_records(fq2)[:rec]) if fq2 else b""
    return len(O.chunk_table(O.encode_file(a, b, paired, cb))) - 1 >= 2


def refusals():
    """the refusing inputs of the circuits, made once: [Refusal], encode refusals first"""
    global _REFUSALS
    if _REFUSALS is not None:
        return _REFUSALS
    import _fuzz
    import _hostile
    made = []

    def sized(name, fq1, fq2, paired, cb):
        """add()'s size rule, on the unmutated text, which the oracle accepts: its image"""
        want = O.encode_file(fq1, fq2, paired, cb)
        size, chunks = len(fq1) + len(fq2), len(O.chunk_table(want)) - 1
        assert 100_000 <= size <= 350_000 and 2 <= chunks <= 6 and 10_000 <= cb <= 30_000, (name, size, chunks, cb)
        return want

    def enc(name, src, exit, good, bad, paired, cb, late=None, code=RFQ_E_DATA, phrase=None, quotes_150=False):
        sized(name, good[0], good[1], paired, cb)
        said = _oracle_refuses(bad[0], bad[1], paired, cb)
        assert said is not None, "%s: the oracle encodes the mutated text" % name
        if quotes_150:                                                       # (oracle/rfq_oracle.c quotes 150 bases of the offending line, the reference all of it: the
            assert len(said.split("\n")[-1]) == 150                          # oracle's whole text is then the phrase the message must hold)
            phrase = said
        if late is not None:
            assert _late(good[0], good[1], paired, cb, late), "%s: record %d is not behind two chunks" % (name, late)
        assert phrase is None or phrase in said, (name, phrase, said)
        made.append(_refusal(name, "enc", src, exit, (code,), message=None if phrase else said, phrase=phrase, fq1=bad[0], fq2=bad[1], paired=paired, cb=cb))

    def one_byte(fq, rec, line, at, byte):
        recs = _records(fq); b = bytearray(recs[rec][line]); b[at] = byte; recs[rec][line] = bytes(b)
        return _text(recs)

    def coord(fq, rec, axis):
        recs = _records(fq); recs[rec][0] = _with_coord(recs[rec][0], axis, COORD_MAX)
        return _text(recs)

    # --- enc_verdict: the coordinate range, found by the coders behind every kernel of the batch, in the LAST chunk
    i = by_name("four_quals"); n = len(_records(i.fq1))
    enc("coord_late_masks", "four_quals", "enc_verdict: planes, room repeat, header made", (i.fq1, b""), (coord(i.fq1, n - 5, 5), b""), O.SE, i.cb, late=n - 5)
    a, b = O.gen(O.NOVA_PE150, 400, seed=11, nppm=20000)                     # (pe150's pairs with N bases in most reads: the loose slots' N bits are stored)
    assert a.count(b"N") > 1000 and len(a) == len(b)
    i = by_name("pe150")
    enc("coord_late_pe", "pe150 with N bases", "enc_verdict: mirrored index, the loose slots' N bits", (a, b), (coord(a, 395, 6), coord(b, 395, 6)), O.PE_TWO_FILES, i.cb,
        late=395)
    # (bgi_q40's names hold no coordinates - there is no X or Y to be out of range -: its reads and forty quality values under NovaSeq names)
    i = by_name("bgi_q40")

    def renamed(fq, mate):
        recs = _records(fq)
        for k, r in enumerate(recs):
            r[0] = b"@A00250:26:H3YTWDSXX:1:%d:%d:%d %d:N:0:ACGT" % (1101 + k // 150, 1000 + 61 * k % 29000, 1000 + 13 * (k % 150), mate)
        return _text(recs)
    a, b = renamed(i.fq1, 1), renamed(i.fq2, 2)
    h = _sections.Header(O.encode_file(a, b, O.PE_TWO_FILES, 20000))
    assert len(h.normal) >= 5 and h.flags & _sections.H_QUAL_BY_COL and not h.flags & _sections.H_DONT_QUAL, (len(h.normal), hex(h.flags))   # (rfq_encode.hip, enc_form: coder_list)
    enc("coord_late_list", "bgi_q40 under NovaSeq names", "enc_verdict: the list coder", (a, b), (coord(a, 445, 6), coord(b, 445, 6)), O.PE_TWO_FILES, 20000, late=445)
    # --- header_errors: chunk 0's bases and qualities
    i = by_name("rare_quals")
    enc("lowercase_chunk0", "rare_quals", "header_errors, tile path", (i.fq1, b""), (one_byte(i.fq1, 40, 1, 70, ord("a")), b""), O.SE, i.cb)
    # (rfq_encode.hip, enc_form: the tile gather takes a batch when two of its longest records and 64 bytes fit G2_CAP = 23552 bytes of staged text - records of more
    # than 11744 bytes go to the byte-wise gather, whose header verdict is read behind it)
    a = E.handmade(20, lambda k: "LR.%d" % k, lambda k: 6000 + 7 * k, lambda k: "+", seed=9)
    assert max(len(b"\n".join(r)) + 1 for r in _records(a)) * 2 + 64 > 23552
    enc("iupac_chunk0_long", "twenty reads of 6000 bases and more", "header_errors behind the byte-wise gather", (a, b""), (one_byte(a, 1, 1, 3000, ord("R")), b""),
        O.SE, 30000, quotes_150=True)
    i = by_name("se_var"); q = _records(i.fq1)[30][3]
    enc("bad_qual_chunk0", "se_var", "header_errors: mixed lengths", (i.fq1, b""), (one_byte(i.fq1, 30, 3, len(q) // 2, 0x85), b""), O.SE, i.cb)
    # --- enc_cut
    i = by_name("se150_big"); recs = _records(i.fq1); n = len(recs); recs[n - 7][3] = recs[n - 7][3][:-1]
    enc("qual_short_late", "se150_big", "enc_cut, RFQ_E_UNPINNED", (i.fq1, b""), (_text(recs), b""), O.SE, i.cb, late=n - 7, code=RFQ_E_UNPINNED, phrase="shorter than")
    # --- enc_verdict: no room in the caller's buffer (nothing is wrong with the text: the code alone)
    i = by_name("long_names")
    made.append(_refusal("nospace", "enc", "long_names", "enc_verdict, RFQ_E_NOSPACE", (RFQ_E_NOSPACE,), fq1=i.fq1, paired=i.paired, cb=i.cb, short=len(i.want) - 1))
    # --- enc_verdict: a quality payload beyond the reference's 1.5x buffer.  _fuzz.qual_case(12) is the first seed of a _fuzz generator (of range(200), at 30,000 bases
    # a chunk) whose text has the size and that the oracle refuses so; there is no unmutated text, so the size rule's chunk count has nothing to count
    fq1, fq2, paired, _ = _fuzz.qual_case(QUAL_OVERFLOW_SEED)
    said = _oracle_refuses(fq1, fq2, paired, 30000)
    assert 100_000 <= len(fq1) + len(fq2) <= 350_000 and said and "1.5x scratch buffer" in said, (len(fq1) + len(fq2), said)
    made.append(_refusal("qual_overflow", "enc", "_fuzz.qual_case(%d)" % QUAL_OVERFLOW_SEED, "enc_verdict: the 1.5x quality payload", (RFQ_E_UNPINNED,),
                         phrase="1.5x scratch buffer", fq1=fq1, fq2=fq2, paired=paired, cb=30000))

    # --- decode: mutants of history images, chosen by the label _hostile.mutants(want, seed=7) gives them; the oracle refuses each
    def mutant(name, src, exit, pick):
        i = by_name(src); muts = _hostile.mutants(i.want, seed=7)
        label, img, index = pick(i, muts)
        MUTANT_LABELS[name] = (src, label)
        if index is None:
            try:
                O.decode_file(img, i.split)
            except O.OracleError:
                made.append(_refusal(name, "dec", src, exit, sorted(_hostile.ALLOWED), image=img, split=i.split))
                return
            raise AssertionError("%s: the oracle decodes mutant %s of %s" % (name, label, src))
        assert img == i.want and list(index) != O.chunk_table(i.want)
        made.append(_refusal(name, "dec", src, exit, (), image=img, split=i.split, chunk_off=list(index), text=i.text))

    def labelled(label):
        return lambda i, muts: next(m for m in muts if m[0] == label)

    def last_chunk_cut(i, muts):
        _, chunks = _sections.parse(i.want); c = chunks[-1]
        return labelled("truncate@%d" % (c.off + c.qual_off))(i, muts)       # (the last chunk's sequence section ends here, its quality payload is missing)
    mutant("cut_last_chunk", "four_quals", "a truncation at a section boundary of the last chunk", last_chunk_cut)
    mutant("scribbled_lengths", "se_var", "a scribbled length table", labelled("lengths15@10642"))
    mutant("scribbled_quality", "rare_quals", "a scribbled quality table", labelled("quality0@11597"))
    mutant("lying_index", "pe150", "a lying chunk index", labelled("index0"))
    i = by_name("se150_big")
    try:
        O.decode_file(i.want, True)
        raise AssertionError("the oracle splits an SE image")
    except O.OracleError as e:
        made.append(_refusal("se_split", "dec", "se150_big", "an SE image with split_pe", (RFQ_E_DATA,), message=str(e), image=i.want, split=True))
    i = by_name("long_names")
    made.append(_refusal("text_nospace", "dec", "long_names", "the speculative emitter, RFQ_E_NOSPACE", (RFQ_E_NOSPACE,), image=i.want, caps=(len(i.text) - 1, 0)))
    assert len({m.name for m in made}) == len(made)
    _REFUSALS = made
    return made


def refusal(name):
    return next(r for r in refusals() if r.name == name)


def refuse_step(codec, r):
    """'' or what is wrong with what the context says to a refusing input"""
    from repaq_amd import RfqError
    try:
        if r.kind == "enc" and r.short is None:
            got = E.encode(codec, r.fq1, r.fq2, r.paired, r.cb)
        elif r.kind == "enc":
            codec.clearHeader()
            d = codec.dev_put(r.fq1); out = codec.dev_put(b"\0" * r.short)
            try:
                assert r.paired == O.SE and out.value % 16 == 0
                res = codec.encode(d, len(r.fq1), None, 0, r.paired, r.cb, d_out=out, out_cap=r.short, **E.nolb_args(r.fq1, r.fq2, r.paired))
                got = codec.dev_get(res.d_rfq, res.rfq_len)
            finally:
                codec.dev_free(d); codec.dev_free(out)
        else:
            got = codec.decode_bytes(r.image, split_pe=r.split, out_caps=r.caps, **({"chunk_off": r.chunk_off} if r.chunk_off else {}))
    except RfqError as e:
        if r.text is not None:
            return "refused (%d: %s) what it must decode" % (e.code, e.message.strip()[:120])
        if e.code not in r.codes:
            return "code %d (%s) for one of %s" % (e.code, e.message.strip()[:120], list(r.codes))
        if r.message is not None and e.message.strip() != r.message.strip():
            return "the message is %r, the oracle's %r" % (e.message.strip()[:200], r.message.strip()[:200])
        if r.phrase is not None and r.phrase not in e.message:
            return "the message %r lacks %r" % (e.message.strip()[:200], r.phrase)
        return ""
    if r.text is None:
        return "a result (%d bytes) instead of the refusal" % (sum(len(x) for x in got) if isinstance(got, tuple) else len(got))
    return (text_diff(got[0], r.text[0]) or text_diff(got[1], r.text[1])) if r.split else text_diff(got, r.text)


def marks_ok(marks, rules):
    return all((r[1:] not in marks) if r.startswith("!") else (r in marks) for r in rules)


# ---------------------------------------------------------------- where two images differ
def where(want: bytes, off: int):
    """(chunk, section) of the oracle's image `want` that byte `off` lies in"""
    try:
        h, chunks = _sections.parse(want)
    except Exception as e:                                                   # (the message must not get lost in a second failure)
        return "?", "unparsed (%s)" % e
    if off < h.len:
        return "-", "header"
    for k, c in enumerate(chunks):
        if c.off <= off < c.off + c.total:
            r = off - c.off
            ends = (("sizes", c.fixed), ("length arrays", c.len_arrays_end), ("lane/tile/x/y", c.coords_end), ("names/strand", c.qual_off - c.seq_size),
                    ("sequence", c.qual_off), ("quality", c.qual_off + c.qual_size), ("overlap/N positions", c.total))
            return k, next(name for name, end in ends if r < end)
    return "?", "behind the last chunk"


def first_diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    if a[:n] == b[:n]:
        return n
    x = np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n)
    return int(np.argmax(x))


def image_diff(got: bytes, want: bytes):
    """'' when equal; otherwise the first differing offset and the chunk and section of the oracle's image it lies in"""
    if got == want:
        return ""
    off = first_diff(got, want)
    chunk, section = where(want, off)
    return "%d bytes for %d, first difference at offset %d: chunk %s, section %s" % (len(got), len(want), off, chunk, section)


def text_diff(got: bytes, want: bytes):
    if got == want:
        return ""
    off = first_diff(got, want)
    return "%d bytes for %d, first difference at offset %d (record %d)" % (len(got), len(want), off, want[:off].count(b"\n") // 4)


# ---------------------------------------------------------------- one step of a circuit
def encode_step(codec, inp):
    """'' or what is wrong with the context's image of the input"""
    got = E.encode(codec, inp.fq1, inp.fq2, inp.paired, inp.cb)
    return image_diff(got, inp.want)


def decode_step(codec, inp):
    """'' or what is wrong with the context's text(s) of the oracle's image"""
    caps = None
    if inp.caller:
        caps = (len(inp.text[0]) + 64, len(inp.text[1]) + 64) if inp.split else (len(inp.text) + 64, 0)
    got = codec.decode_bytes(inp.want, split_pe=inp.split, out_caps=caps)
    if inp.split:
        return text_diff(got[0], inp.text[0]) or text_diff(got[1], inp.text[1])
    return text_diff(got, inp.text)


def check_markers(make_codec, inp):
    """the input reaches the state it is there for: on a fresh context the first encode / decode (and the second encode) shows its stage markers, and every result is the oracle's"""
    c = make_codec()
    try:
        bad = encode_step(c, inp)
        marks = {n for n, _ in c.timings()}
        assert not bad, (inp.name, bad)
        assert marks_ok(marks, inp.enc_mark), (inp.name, inp.enc_mark, sorted(marks))
        if inp.enc2_mark:
            bad = encode_step(c, inp)
            marks = {n for n, _ in c.timings()}
            assert not bad, (inp.name, "second encode", bad)
            assert marks_ok(marks, inp.enc2_mark), (inp.name, "second encode", inp.enc2_mark, sorted(marks))
    finally:
        c.close()
    c = make_codec()
    try:
        bad = decode_step(c, inp)
        marks = {n for n, _ in c.timings()}
        assert not bad, (inp.name, bad)
        assert marks_ok(marks, inp.dec_mark), (inp.name, inp.dec_mark, sorted(marks))
    finally:
        c.close()


def walk(codec, seq, kind_of, start=0, stop=None, state=None, nodes=None):
    """steps start .. stop of the sequence on `codec`; kind_of(i) -> "enc" / "dec".  Every failing step is collected (the context goes on: what a wrong state does to
    the calls behind it is part of the picture) and the assert names the input, the call in front of it and - encode state is left by the last ENCODE, decode state
    by the last decode - the last call of its own kind, with the place.  state: what walk returned for the steps in front of `start` on this context.
    nodes: what seq indexes, inputs() by default; a Refusal among them is an encode or a decode by its own kind and passes when the context raises what it expects
    (refuse_step) - a result, another code or another message is collected like a differing image."""
    from repaq_amd import RfqError
    ins = inputs() if nodes is None else nodes; bad = []
    state = dict(state or {})
    stop = len(seq) if stop is None else stop
    for i in range(start, stop):
        inp = ins[seq[i]]
        if isinstance(inp, Refusal):
            kind = inp.kind; msg = refuse_step(codec, inp)
        else:
            kind = kind_of(i)
            try:
                msg = (encode_step if kind == "enc" else decode_step)(codec, inp)
            except RfqError as e:                                            # (what an earlier refusal left behind may well be a refusal of a good input)
                msg = "refused (%d: %s)" % (e.code, e.message.strip()[:120])
        if msg:
            marks = sorted(n for n, _ in codec.timings())
            prev, same = state.get("prev"), state.get(kind)
            behind = (prev or "a fresh context") + ("" if same == prev else ", the last %s being %s" % (kind, same or "none"))
            bad.append("step %d: %s of %s behind %s: %s; stages %s" % (i, kind, inp.name, behind, msg, marks))
        state["prev"] = state[kind] = "%s of %s" % (kind, inp.name)
    assert not bad, "%d of %d steps differ from the oracle:\n%s" % (len(bad), stop - start, "\n".join(bad[:12]))
    return state


KINDS = {"encode": lambda i: "enc", "decode": lambda i: "dec", "mixed": lambda i: "enc" if i % 2 else "dec"}


def refusal_circuit(kind):
    """(nodes, seq, G, R) of the refusal circuit `kind`: the good inputs and the refusing ones of that kind (both kinds' for "mixed"), every ordered pair of them adjacent
    once but good -> good, which the circuits over inputs() alone have"""
    good = list(inputs()); ref = [r for r in refusals() if kind == "mixed" or r.kind == {"encode": "enc", "decode": "dec"}[kind]]
    g, r = len(good), len(ref)
    seq = circuit(range(g + r), refusal_edges(g, r))
    assert len(seq) == 2 * g * r + r * r + 1, (kind, g, r, len(seq))
    return good + ref, seq, g, r


def check_fast_path_kept(codec):
    """behind a circuit with refusals on `codec`: a uniform file twice, and the second encode is indexed without the read-back (check_mixed_lengths_end_with_the_file's
    assertion) - no refusal costs the context its fast path for good"""
    inp = by_name("se150_big")
    for _ in range(2):
        msg = encode_step(codec, inp)
        assert not msg, msg
        marks = {n for n, _ in codec.timings()}
    assert "lazy_index" in marks, sorted(marks)


def check_header_survives_refusal(codec):
    """The file in progress behind a refusal at the encoder's LAST exit, without rfq_clear_header.  include/rfq_hip.h gives a refusal no say over the header ("the header
    currently set / made", rfq_get_header; only rfq_clear_header, rfq_set_header and a decode with has_header change it), and enc_verdict refuses behind the header stage:
    the header made from the refused text's chunk 0 stays.  It equals the oracle's header of the unmutated text - the mutation lies behind chunk 0, or nowhere (nospace) -
    and the unmutated text encoded next, as the file in progress, is that header and the oracle's chunks behind it."""
    for name in ("coord_late_masks", "nospace"):
        r = refusal(name); good = by_name(r.src)
        hdr = good.want[:_sections.Header(good.want).len]
        msg = refuse_step(codec, r)
        assert not msg, (name, msg)
        got = codec.header()
        assert got == hdr, (name, got.hex(), hdr.hex())
        image = codec.encode_bytes(good.fq1, good.fq2, good.paired, good.cb, **E.nolb_args(good.fq1, good.fq2, good.paired))     # (no clearHeader in front)
        assert image == good.want, (name, image_diff(image, good.want))
        assert codec.header() == hdr, name


# ---------------------------------------------------------------- one file in two batches
def check_two_batches(codec, inp, other):
    """`inp` (one text) split at a record boundary: the first half with final=False, flush_all=True, a decode of `other`'s image on the same context, the second half
    with emit_header=False - the concatenation is the oracle's image of the whole text.  The boundary is the record at which the oracle's image ends a chunk (the one
    nearest the middle): flush_all ends a chunk where the batch ends, so at any other record the two batches make a valid image of the text, but not the oracle's."""
    from repaq_amd import nolb_threshold
    assert inp.paired == O.SE and b"\r" not in inp.fq1
    _, chunks = _sections.parse(inp.want)
    assert len(chunks) >= 2
    recs = _records(inp.fq1); cut = len(_text(recs[:sum(c.reads for c in chunks[:len(chunks) // 2])]))
    assert 0 < cut < len(inp.fq1)
    th = nolb_threshold(len(inp.fq1), inp.fq1.endswith(b"\n"))
    codec.clearHeader()
    d = codec.dev_put(inp.fq1[:cut])
    try:
        r = codec.encode(d, cut, None, 0, O.SE, inp.cb, final=False, flush_all=True, nolb_from1=th)
        assert r.consumed1 == cut, (r.consumed1, cut)
        first = codec.dev_get(r.d_rfq, r.rfq_len)
    finally:
        codec.dev_free(d)
    hdr = codec.header()
    msg = decode_step(codec, other)
    assert not msg, (other.name, msg)
    # (a decode with has_header parses the image's header and SETS it - include/rfq_hip.h, rfq_decode_args - so the file in progress takes its own back, the way a
    # worker of the host queue takes the first range's: rfq_get_header -> rfq_set_header.  What the context knew about the file is gone with it: new_file())
    assert codec.header() != hdr
    codec.setHeader(hdr)
    d = codec.dev_put(inp.fq1[cut:])
    try:
        r = codec.encode(d, len(inp.fq1) - cut, None, 0, O.SE, inp.cb, emit_header=False, file_off1=cut, nolb_from1=th)
        second = codec.dev_get(r.d_rfq, r.rfq_len)
    finally:
        codec.dev_free(d)
    return first + second


# ---------------------------------------------------------------- threads
def run_threads(jobs, timeout_s=120.0):
    """every job (a callable) on a host thread of its own, released together; an exception of any thread is raised here, a thread that does not come back fails"""
    barrier = threading.Barrier(len(jobs)); errors = [None] * len(jobs)

    def body(i):
        try:
            barrier.wait(timeout_s)
            jobs[i]()
        except BaseException as e:                                           # noqa: BLE001 (handed to the main thread)
            errors[i] = e
    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(jobs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout_s)
    hung = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not hung, "threads %s did not come back within %.0f s" % (hung, timeout_s)
    for i, e in enumerate(errors):
        if e is not None:
            raise AssertionError("thread %d: %s: %s" % (i, type(e).__name__, e)) from e


# ---------------------------------------------------------------- the calls circuit: every KIND of call behind every other one
# One fixed small input per kind.  Every call goes through the helper its own tests use, which compares it with a host loop or the oracle EVERY time; what it returns
# (every output's bytes) must also equal what the same call gave first.  Context-owned results (rfq_decode_names' names_blob / names_off, rfq_rows_to_text's rows_txt,
# the encoder's and decoder's own result buffers): include/rfq_hip.h says "result pointers stay valid until the next call on the same context" - the next call
# invalidates them, so each is read BEFORE the next kind's call is issued, inside its own step.
CALL_KINDS = ("encode", "decode", "scan", "first_diff", "decode_rows", "decode_names", "text_rows", "select_rows", "judge_rows", "adapter_rows", "merge_rows",
              "rows_to_text", "encode_rows", "dedup_rows", "profile_rows", "screen_rows", "kmers_rows", "demux_rows", "group_rows")

# The entry points of include/rfq_hip.h a kind's step calls (beside the memory helpers every step uses).  tests/test_call_kinds.py holds this list against the
# library's exports: an entry point that is in no step and not in NOT_A_CALL_KIND fails there by name, so the next one cannot stay out of the circuits unnoticed.
KIND_ENTRY_POINTS = {
    "encode": ("rfq_encode_batch",), "decode": ("rfq_decode_batch",), "scan": ("rfq_scan_batch",), "first_diff": ("rfq_compare_bytes",),
    "decode_rows": ("rfq_decode_rows",), "decode_names": ("rfq_decode_names",), "text_rows": ("rfq_text_rows",), "select_rows": ("rfq_select_rows",),
    "judge_rows": ("rfq_judge_rows",), "adapter_rows": ("rfq_adapter_rows",), "merge_rows": ("rfq_merge_rows",), "rows_to_text": ("rfq_rows_to_text",),
    "encode_rows": ("rfq_encode_rows",), "dedup_rows": ("rfq_dedup_rows",), "profile_rows": ("rfq_profile_rows",),
    "screen_rows": ("rfq_screen_build", "rfq_screen_rows"),
    "kmers_rows": ("rfq_kmers_init", "rfq_kmers_rows", "rfq_kmers_read", "rfq_screen_rows"),      # (the read's index is screened with: that is what it is for)
    "demux_rows": ("rfq_demux_rows",), "group_rows": ("rfq_group_rows",),
}
NOT_A_CALL_KIND = (
    ("rfq_create", "makes the context every step runs on"), ("rfq_destroy", "ends it"), ("rfq_last_error", "read by every refusing step: the message"),
    ("rfq_set_stream", "which stream the calls run on: tests/test_*_api.py"),
    ("rfq_set_header", "the file in progress: check_two_batches"), ("rfq_get_header", "check_two_batches, check_header_survives_refusal"),
    ("rfq_clear_header", "in front of every encode step"),
    ("rfq_last_timings", "read behind steps: the stage markers"), ("rfq_version", "a constant string"),
    ("rfq_set_option", "a switch, not a call on data: test_switches_stay_with_their_context"), ("rfq_get_option", "reads a switch"),
    ("rfq_option_name", "lists the switches"),
    ("rfq_dev_malloc", "memory helper: every step's buffers"), ("rfq_dev_free", "memory helper"), ("rfq_copy_h2d", "memory helper: every step's inputs"),
    ("rfq_copy_d2h", "memory helper: every step's results"), ("rfq_copy_d2d", "memory helper"), ("rfq_copy_peer", "memory helper between two contexts"),
    ("rfq_copy_h2d_async", "memory helper: the host queue's uploads"), ("rfq_copy_done", "asks after such an upload"), ("rfq_copy_sync", "waits for them"),
    ("rfq_host_alloc", "pinned host memory"), ("rfq_host_free", "pinned host memory"), ("rfq_host_register", "pins the caller's"),
    ("rfq_host_unregister", "unpins it"),
    ("rfq_selftest_wave", "a self-test of the wave primitives: keeps nothing on the context"),
)
# what a fresh context's codec.timings() must show of each of these kinds (the stage names of rfq_encode.hip), collected over the calls of its step: first_results
CALL_STAGES = {"profile_rows": ("profile:rows",), "screen_rows": ("screen:build", "screen:rows"), "kmers_rows": ("kmers:init", "kmers:rows", "kmers:read"),
               "demux_rows": ("demux:rows",), "group_rows": ("group:judge", "group:rank", "group:tables", "group:rows", "group:names")}


def _items(d):
    """a dict as something that compares with =="""
    return tuple(sorted(d.items()))


def _slots_of(values):
    """the non-empty slots of a screen index of these canonical values, in ascending order (include/rfq_hip.h, rfq_screen_build: "a slot is 0 (empty) or bit 63 | value")"""
    return np.array(sorted(v | 1 << 63 for v in values), np.uint64).tobytes()


def _index_set(body):
    """What include/rfq_hip.h defines of a screen index's bytes: the 64-byte header, and the SET of the slots behind it - "WHICH slot a value lands in may depend on the
    order of arrival: the index BYTES are private and may differ from run to run".  So an index comes back as (header, non-empty slots in ascending order)."""
    slots = np.frombuffer(body[64:], np.uint64)
    return body[:64], np.sort(slots[slots != 0]).tobytes()


def _note(codec, marks):
    if marks is not None:
        marks.update(n for n, _ in codec.timings())


class Calls:
    """the fixtures of the calls circuit and their host references, made once"""
    def __init__(self):
        import _adapter as A
        import _dedup as D
        import _demux as X
        import _group as G
        import _judge as J
        import _kmers as K
        import _merge as M
        import _names as N
        import _profile as P
        import _rows as W
        import _rows_enc as R
        import _screen as Sc
        import _select as S
        import _text_rows as T
        self.mod = dict(A=A, D=D, J=J, M=M, N=N, W=W, R=R, S=S, T=T, P=P, Sc=Sc, K=K, X=X, G=G)
        self.fq1, self.fq2 = O.gen(O.NOVA_PE150, 70, seed=21)
        self.paired, self.cb = O.PE_TWO_FILES, 10000
        self.want = O.encode_file(self.fq1, self.fq2, self.paired, self.cb)
        assert O.decode_file(self.want, True) == (self.fq1, self.fq2) and len(O.chunk_table(self.want)) - 1 >= 3
        # scan: a chunk ends where its last record ends in each file (the oracle's image says how many reads each chunk holds: both mates' together)
        _, chunks = _sections.parse(self.want)
        nl1 = [i + 1 for i, c in enumerate(self.fq1) if c == 10]; nl2 = [i + 1 for i, c in enumerate(self.fq2) if c == 10]
        pairs = np.cumsum([c.reads // 2 for c in chunks])
        self.scan_want = (len(chunks), [nl1[4 * int(p) - 1] for p in pairs], [nl2[4 * int(p) - 1] for p in pairs])
        # first_diff: two texts that differ in one byte behind the first 64 KiB
        self.cmp_a = self.fq1 * 4; self.cmp_at = 70_001
        b = bytearray(self.cmp_a); b[self.cmp_at] ^= 1; self.cmp_b = bytes(b)
        self.rows_want = W.expected(self.want)
        self.names_want = N.expected(self.want)
        self.recs = T.expect(self.fq1, self.fq2, self.paired, self.cb)[1]
        self.rows = R.rows_of(self.fq1, self.fq2, self.paired, extra="x16")
        B, Q, lens, names = self.rows; n = len(lens); rng = np.random.default_rng(31)
        self.sel = dict(keep=(rng.random(n) < 0.8).astype(np.uint8), start=rng.integers(0, 20, n).astype(np.int32), length=rng.integers(0, 120, n).astype(np.int32),
                        pairs=True, min_len=30)
        self.j_rows = J.random_rows(257, 150, 41, codes=False); self.j_crit = dict(J.STEPS)["all"]
        self.j_want = J.expected(*self.j_rows, self.j_crit, False)
        self.a_rows = A.random_pairs(33, 150, 43, codes=True); self.a_crit = A.shape_criteria(150)[2][1]
        self.a_want = A.expected(*self.a_rows, self.a_crit, True)
        self.m_rows = M.random_pairs(40, 64, 47, codes=False)
        self.m_want = M.expected(*self.m_rows, False)
        self.d_rows = D.planted(100, True, 53, sizes=(20, 5, 2) + (1,) * 40)
        self.d_want = D.expected(*self.d_rows, pairs=True, best=True, hist_len=8)
        self._make_profile(P); self._make_screen(Sc); self._make_kmers(K, Sc); self._make_demux(X); self._make_group(G)
        # --- what the refusing kinds send (REFUSING_CALL_KINDS): each a fixture above with the ONE mutation its own module's refusal tests make
        import _hostile
        self.code_rows = R.rows_of(self.fq1, self.fq2, self.paired, extra="x16", codes=True)
        self.code_rows[0][3, 70] = 5                                          # (_rows_enc._refusals: code_5_mid_line)
        self.junk = dict(T.junk_texts())["nul_and_ff"]                        # (a NUL and a 0xFF in a sequence line: no base code for them, include/rfq_hip.h, rfq_text_rows)
        label, img, split, _ = _hostile.images()[0]                           # (se150: the image whose mutants _rows.run_hostile / _names.run_hostile send)
        _, chunks = _sections.parse(img); cut = "truncate@%d" % (chunks[-1].off + chunks[-1].qual_off)
        self.mutant = next(m for m in _hostile.mutants(img, seed=7) if m[0] == cut)[1]
        try:
            O.decode_file(self.mutant, split)
            raise AssertionError("the oracle decodes %s of %s" % (cut, label))
        except O.OracleError:
            pass
        fq = _qual_recs(260, b"F:,5", 5); recs = _records(fq); recs[-5][0] = _with_coord(recs[-5][0], 5, COORD_MAX)
        self.se_want = O.encode_file(fq, b"", O.SE, self.cb)
        assert len(O.chunk_table(self.se_want)) - 1 >= 3 and _late(fq, b"", O.SE, self.cb, len(recs) - 5)
        self.coord_fq = _text(recs); self.coord_said = _oracle_refuses(self.coord_fq, b"", O.SE, self.cb)
        assert self.coord_said == "The X/Y coordinate cannot be larger than 2M, but we get: %d" % COORD_MAX, self.coord_said
        try:
            O.decode_file(self.se_want, True)
            raise AssertionError("the oracle splits an SE image")
        except O.OracleError as e:
            self.split_said = str(e)

    # --- the fixtures of the five kinds behind dedup: each the smallest that still takes the call's default kernel with more than one workgroup (or wave) at work
    def _make_profile(self, P):
        """129 pairs at row_len 150 under a keep / start / length triple: the LDS kernel, 16 units a workgroup's step"""
        B, Q, lens = P.random_rows(258, 150, 71, codes=False)
        start, length = P.random_windows(lens, 72)
        keep = (np.random.default_rng(73).random(258) < 0.8).astype(np.uint8)
        self.p_rows = (B, Q, lens, keep, start, length); self.p_kw = dict(pairs=True, cycles=150, qbins=64, len_bins=151)
        self.p_want = P.expected(B, Q, lens, False, True, keep, start, length, 150, 64, 151)
        assert min(self.p_want["summary"]["counted"]) > 50 and self.p_want["summary"]["max_len"] > 100
        assert P.BAD["window_past_the_read"] == ("length", "l+1")             # (_profile.check_device_refusal: length = lens - start + 1, here in the last row)
        bad = length.copy(); bad[-1] = lens[-1] - start[-1] + 1
        self.p_bad = (B, Q, lens, keep, start, bad)

    def _make_screen(self, Sc):
        """two references, k = 21; 65 pairs at row_len 150, every other row with a stretch of a reference (one in four of those reverse-complemented)"""
        rng = np.random.default_rng(74); k = 21
        self.s_refs = [Sc.rand_seq(rng, 300), Sc.rand_seq(rng, 260)]; self.s_k = k
        seqs = []
        for i in range(130):
            l = int(rng.integers(60, 151)); s = bytearray(Sc.rand_seq(rng, l))
            if i % 2 == 0:
                ref = self.s_refs[(i // 2) % 2]; w = int(rng.integers(k, 50)); at = int(rng.integers(0, len(ref) - w + 1))
                piece = ref[at:at + w] if i % 8 else Sc.revcomp(ref[at:at + w])
                p = int(rng.integers(0, l - w + 1)); s[p:p + w] = piece
            seqs.append(bytes(s))
        self.s_rows = Sc.rows_of(seqs, 150, "ascii", seed=75); self.s_kw = dict(pairs=True, min_hits=2, min_pct=10)
        self.s_set = Sc.ref_set(self.s_refs, k)[0]
        self.s_want = Sc.expected(*self.s_rows, self.s_set, k, False, **self.s_kw)
        s = self.s_want["summary"]
        assert 10 < s["n_matched"] < 65 and s["n_kept"] == 65 - s["n_matched"] and int((self.s_want["hits"] == 1).sum()) > 0, s
        self.s_slots = _slots_of(self.s_set)

    def _make_kmers(self, K, Sc):
        """k = 17; 130 rows at row_len 150 in two calls of 64 and 66: three in four are stretches of one sequence of 1500 bases (either strand), so that values
        come back within a call and in the second call, the others are of their own; an N in every tenth"""
        rng = np.random.default_rng(76); k = 17
        genome = Sc.rand_seq(rng, 1500); seqs = []
        for i in range(130):
            l = int(rng.integers(40, 151))
            if i % 4 == 3:
                s = Sc.rand_seq(rng, l)
            else:
                at = int(rng.integers(0, 1500 - l + 1)); s = genome[at:at + l] if i % 3 else Sc.revcomp(genome[at:at + l])
            s = bytearray(s)
            if i % 10 == 0:
                s[l // 2] = ord("N")
            seqs.append(bytes(s))
        B, lens = Sc.rows_of(seqs, 150, "ascii", seed=77)
        self.k_k = k; self.k_rows = ((B[:64], lens[:64]), (B[64:], lens[64:]))
        (c1, km1, s1), (c2, km2, s2) = (K.model(b, l, k, False) for b, l in self.k_rows)
        self.k_cnt = c1 + c2
        self.k_want = [(km1, dict(s1, n_new=len(c1), n_kmers=len(c1), total=sum(c1.values()), lost=0)),
                       (km2, dict(s2, n_new=len(set(c2) - set(c1)), n_kmers=len(self.k_cnt), total=sum(self.k_cnt.values()), lost=0))]
        sel = {v for v, _ in K.selected(self.k_cnt, 2)}
        # (more values than the smallest table has slots: kmers_full; values the second call adds to and values it brings; values that stay below min_count)
        assert len(self.k_cnt) > 2048 and set(c1) & set(c2) and set(c2) - set(c1) and 200 < len(sel) < len(self.k_cnt) - 200, (len(self.k_cnt), len(sel))
        self.k_sel_slots = _slots_of(sel)
        self.k_screen = Sc.expected(*self.k_rows[1], sel, k, False)          # (the read's index, screened with: the second call's rows)
        assert 0 < self.k_screen["summary"]["n_matched"] < 66

    def _make_demux(self, X):
        """two sets of 8 and 6 barcodes of 8 bases, a sheet of some of the 48 combinations; 66 pairs at row_len 64: _demux.pair_rows' units - every combination
        exact, and every reason alone -, the ambiguous read _demux.check_pairs plants, and pairs of random bases"""
        rng = np.random.default_rng(78); L = 64; off = (X.COMPOSE["off1"], X.COMPOSE["off2"])
        set1 = X.distinct_barcodes(rng, 7, 8, min_dist=4); set2 = X.distinct_barcodes(rng, 6, 8, min_dist=4)
        amb = X.mutate(set1[0], 2); set1 = set1 + [X.mutate(amb, 5)]          # (set1[7] is 2 from set1[0]: `amb` is 1 from both)
        every = [(i, j) for i in range(8) for j in range(6)]
        sheet = [(0, 0)] + [every[k] for k in rng.permutation(48)[:20] if every[k] != (0, 0)]
        seqs, lens = X.pair_rows(rng, set1, set2, off, L)
        seqs += [(X.rand_seq(rng, off[0]) + amb + X.rand_seq(rng, 20))[:L], (set2[0] + X.rand_seq(rng, 9))[:L]]; lens += [len(s) for s in seqs[-2:]]
        while len(seqs) < 132:
            seqs.append(X.rand_seq(rng, int(rng.integers(0, L + 1)))); lens.append(len(seqs[-1]))
        self.x_rows = X.rows_of(seqs, L, lens=lens)
        self.x_cfg = X.Cfg(set1, set2, sheet, pairs=True, **X.COMPOSE)
        self.x_want = X.expected(*self.x_rows, self.x_cfg, False)
        s = self.x_want["summary"]
        assert all(s[f] >= 1 for f in ("why_none", "why_ambig", "why_short", "why_combo")) and 0 < s["n_exact"] < s["n_assigned"] and s["n_units"] == 66, s

    def _make_group(self, G):
        """GR_TILE + 1 units at row_len 16, with names: two tiles of the sort; 300 bins and the rest bin: both digit passes"""
        U = G.GR_TILE + 1; rng = np.random.default_rng(79)
        B, Q, lens, names = G.case_rows(U, 16, 79)
        bins = rng.integers(-1, 300, U).astype(np.int32)
        keep = (rng.random(U) < 0.9).astype(np.uint8); start = np.minimum(rng.integers(0, 4, U), lens - 1).astype(np.int32)
        length = (rng.random(U) * (lens - start + 1)).astype(np.int32)
        self.g_rows = (B, Q, lens, names, bins); self.g_bins = 300; self.g_kw = dict(rest=True, keep=keep, start=start, length=length)
        e = G.expected(*self.g_rows, 300, **self.g_kw)
        assert e["used"] > 256 and int(e["bin_off"][300]) < len(e["idx"]) and e["mask"] > 0 and e["short"] > 0 and len(e["idx"]) > 1024, (e["used"], e["mask"], e["short"], len(e["idx"]))
        self.g_bad_unit = 1000
        self.g_bad = bins.copy(); self.g_bad[self.g_bad_unit] = 300           # (_group.check_device_refusal: a bin equal to n_bins)

    # each returns every output's bytes, as something that compares with ==
    def encode(self, c):
        got = E.encode(c, self.fq1, self.fq2, self.paired, self.cb)
        assert got == self.want, image_diff(got, self.want)
        return got

    def decode(self, c):
        got = c.decode_bytes(self.want, split_pe=True)
        assert got == (self.fq1, self.fq2), text_diff(got[0], self.fq1) or text_diff(got[1], self.fq2)
        return got

    def scan(self, c):
        d1 = c.dev_put(self.fq1); d2 = c.dev_put(self.fq2)
        try:
            r, e1, e2 = c.scan(d1, len(self.fq1), d2, len(self.fq2), self.paired, self.cb, final=True)
        finally:
            c.dev_free(d1); c.dev_free(d2)
        got = (r.n_chunks, e1, e2)
        assert got == self.scan_want, (got, self.scan_want)
        return got

    def first_diff(self, c):
        da = c.dev_put(self.cmp_a); db = c.dev_put(self.cmp_b)
        try:
            got = (c.first_diff(da, db, len(self.cmp_a)), c.first_diff(da, da, len(self.cmp_a)), c.first_diff(da, db, self.cmp_at))
        finally:
            c.dev_free(da); c.dev_free(db)
        assert got == (self.cmp_at, len(self.cmp_a), self.cmp_at), got
        return got

    def decode_rows(self, c):
        n, ml, B, Q, lens = self.rows_want
        gn, gml, gb, gq, gl = c.decode_rows_bytes(self.want)
        assert (gn, gml) == (n, ml), "decode_rows: %r rows / longest for %r" % ((gn, gml), (n, ml))
        for what, got, want in (("lengths", gl, lens), ("bases", gb, B), ("qualities", gq, Q)):
            assert np.array_equal(got, want), "decode_rows: %s differ, first in row %d" % (what, int(np.nonzero((got != want).reshape(n, -1).any(axis=1))[0][0]))
        return gn, gml, gb.tobytes(), gq.tobytes(), gl.tobytes()

    def decode_names(self, c):
        return tuple(self.mod["N"].check(c, self.want, want=self.names_want))     # (context-owned names and offsets, fetched inside check: before the next call)

    def text_rows(self, c):
        r, B, Q, lens, names = self.mod["T"].call(c, self.fq1, self.fq2, self.paired, recs=self.recs, extra="x16")
        return (int(r.n_rows), int(r.consumed1), int(r.consumed2)), B.tobytes(), Q.tobytes(), lens.tobytes(), tuple(names)

    def select_rows(self, c):
        return tuple(self.mod["S"].call(c, *self.rows, row_len="x16", **self.sel)[5])

    def judge_rows(self, c):
        J, W = self.mod["J"], self.mod["W"]; dev = W.DevRows(c, *self.j_rows)
        try:
            out, summ, raw = J.run(c, dev, self.j_crit, False)
        finally:
            dev.free()
        J.compare(out, summ, self.j_want, "calls circuit:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def adapter_rows(self, c):
        A, W = self.mod["A"], self.mod["W"]; B, lens = self.a_rows; dev = W.DevRows(c, B, None, lens)
        try:
            out, summ, raw = A.run(c, dev, self.a_crit, True)
        finally:
            dev.free()
        A.compare(out, summ, self.a_want, "calls circuit:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def merge_rows(self, c):
        return tuple(self.mod["M"].call(c, *self.m_rows, False, row_len="x16", paths=(None,), e=self.m_want)[3])

    def rows_to_text(self, c):
        got = c.rows_to_text_bytes(*self.rows, paired=self.paired)               # (context-owned texts, copied out inside: before the next call)
        assert got == (self.fq1, self.fq2), text_diff(got[0], self.fq1) or text_diff(got[1], self.fq2)
        return got

    def encode_rows(self, c):
        c.clearHeader()
        got = c.encode_rows_bytes(*self.rows, paired=self.paired, chunk_bases=self.cb, **E.nolb_args(self.fq1, self.fq2, self.paired))
        assert got == self.want, image_diff(got, self.want)
        return got


    def dedup_rows(self, c):
        D = self.mod["D"]; dev = D.dev_rows(c, *self.d_rows)
        try:
            out, summ, raw = D.run(c, dev, pairs=True, best=True, hist_len=8)
        finally:
            dev.free()
        D.compare(out, summ, self.d_want, "calls circuit:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    # (marks: a set that takes the stage names codec.timings() shows behind every call of the step - first_results)
    def profile_rows(self, c, marks=None, rows=None):
        P = self.mod["P"]; dev = P.dev_rows(c, *(rows or self.p_rows))
        try:
            out, summ, raw = P.run(c, dev, False, **self.p_kw)
            _note(c, marks)
        finally:
            dev.free()
        P.compare(out, summ, self.p_want, "calls circuit:")
        return _items(raw), _items(summ)

    def screen_rows(self, c, marks=None, lens=None):
        """rfq_screen_build into an index of the step's own, then rfq_screen_rows with it; the index comes back as _index_set gives it and is the model's set"""
        Sc = self.mod["Sc"]; idx = Sc.Index(c, self.s_refs, self.s_k)         # (compares the build's result with the model's counts)
        try:
            _note(c, marks)
            index = _index_set(idx.g.body())
            assert index[1] == self.s_slots, "the index holds %d values, the model's set %d, or others" % (len(index[1]) // 8, len(self.s_set))
            dev = Sc.dev_rows(c, self.s_rows[0], self.s_rows[1] if lens is None else lens)
            try:
                out, summ, raw = Sc.run(c, dev, idx, **self.s_kw)
                _note(c, marks)
            finally:
                dev.free()
        finally:
            idx.free()
        Sc.compare(out, summ, self.s_want, "calls circuit:")
        return index, _items(raw), _items(summ)

    def kmers_rows(self, c, marks=None, slots=None):
        """rfq_kmers_init on a table of the step's own, two rfq_kmers_rows into it, rfq_kmers_read: the pairs, the spectrum and the screen index, which
        rfq_screen_rows is then given.  The table's bytes and the order of the pairs are private (include/rfq_hip.h): the pairs come back sorted, the index as
        _index_set gives it.  slots: what kmers_full changes"""
        K, Sc = self.mod["K"], self.mod["Sc"]
        t = K.Table(c, self.k_k, K.pow2(2 * len(self.k_cnt)) if slots is None else slots); gi = None
        try:
            _note(c, marks)
            counted = []
            for (B, ln), (kmers, want) in zip(self.k_rows, self.k_want):
                dev = Sc.dev_rows(c, B, ln)
                try:
                    got, summ, raw = t.count(dev)
                    _note(c, marks)
                finally:
                    dev.free()
                assert np.array_equal(got, kmers), "calls circuit: kmers differ, first in row %d" % int(np.nonzero(got != kmers)[0][0])
                assert summ == want, ("calls circuit:", {f: (summ[f], want[f]) for f in K.ROWS_FIELDS if summ[f] != want[f]})
                counted.append((raw, _items(summ)))
            checked = t.check(hist_len=16, min_count=2, cnt=self.k_cnt, what="calls circuit")      # (the pairs, the spectrum, the header: the model's)
            _note(c, marks)
            got = t.read(min_count=2, index=True); gi = got["index"]
            assert got["pairs"] == checked["pairs"] and got["summary"] == checked["summary"], "the read with an index selects otherwise"
            index = _index_set(gi.body())
            assert index[1] == self.k_sel_slots, "the read's index holds %d values, the model selects %d, or others" % (len(index[1]) // 8, len(self.k_sel_slots) // 8)
            dev = Sc.dev_rows(c, *self.k_rows[1])
            try:
                out, summ, raw = Sc.run(c, dev, None, index=(gi.ptr, gi.n))
            finally:
                dev.free()
            Sc.compare(out, summ, self.k_screen, "calls circuit, the read's index:")
            return tuple(counted), tuple(checked["pairs"]), checked["hist"].tobytes(), _items(checked["summary"]), index, _items(raw), _items(summ)
        finally:
            t.free()
            if gi is not None:
                gi.free()

    def demux_rows(self, c, marks=None, lens=None):
        X = self.mod["X"]; dev = X.dev_rows(c, self.x_rows[0], self.x_rows[1] if lens is None else lens)
        try:
            out, summ, raw = X.run(c, dev, self.x_cfg, False, X.ALL)
            _note(c, marks)
        finally:
            dev.free()
        X.compare(out, summ, self.x_want, "calls circuit:")
        return _items(raw), _items(summ)

    def group_rows(self, c, marks=None):
        G = self.mod["G"]
        e, r, got = G.call(c, *self.g_rows, self.g_bins, per_bin=False, **self.g_kw)       # (a size query and the writing call, both against _group.expected)
        _note(c, marks)
        return G.fields_of(r), _items(got)

    # --- the refusing kinds: each raises AssertionError unless the call is refused with the code, and the fragment of the message, its module's own tests expect
    @staticmethod
    def _refused(codes, fragment, f, exact=False):
        from repaq_amd import RfqError
        try:
            f()
        except RfqError as e:
            assert e.code in codes, "code %d (%s) for one of %s" % (e.code, e.message.strip()[:120], sorted(codes))
            said = e.message.strip()
            assert fragment is None or (said == fragment.strip() if exact else fragment in said), "the message %r for %r" % (said[:200], fragment)
            return "refused"
        raise AssertionError("a result instead of the refusal")

    @staticmethod
    def _too_long(lens, row_len):
        """the lengths with row_len + 1 in the last row, and what the message names"""
        lens = np.array(lens, np.int32); lens[-1] = row_len + 1
        return lens, "first such row: %d)" % (len(lens) - 1)

    def _on_rows(self, c, dev, call):
        try:
            return call(dev)
        finally:
            dev.free()

    def bad_select_rows(self, c):
        S = self.mod["S"]; B, Q, lens, names = self.rows; lens, needle = self._too_long(lens, B.shape[1])
        dev = S.dev_sel(c, B, Q, lens, names, self.sel["keep"], self.sel["start"], self.sel["length"])
        return self._on_rows(c, dev, lambda d: self._refused((-3,), needle, lambda: c.select_rows(*d.args(), pairs=True, min_len=30, **S.sel_of(d))))

    def bad_judge_rows(self, c):
        J, W = self.mod["J"], self.mod["W"]; B, Q, lens = self.j_rows; lens, needle = self._too_long(lens, B.shape[1])
        return self._on_rows(c, W.DevRows(c, B, Q, lens), lambda d: self._refused((-3,), needle, lambda: J.run(c, d, self.j_crit, False)))

    def bad_adapter_rows(self, c):
        A, W = self.mod["A"], self.mod["W"]; B, lens = self.a_rows; lens, needle = self._too_long(lens, B.shape[1])
        return self._on_rows(c, W.DevRows(c, B, None, lens), lambda d: self._refused((-3,), needle, lambda: A.run(c, d, self.a_crit, True)))

    def bad_merge_rows(self, c):
        M = self.mod["M"]; B, Q, lens, names, insert = self.m_rows; lens, needle = self._too_long(lens, B.shape[1])
        dev = M.dev_merge(c, B, Q, lens, names, insert)
        return self._on_rows(c, dev, lambda d: self._refused((-3,), needle, lambda: c.merge_rows(*d.args(), d_insert=d.insert, codes=False)))

    def bad_dedup_rows(self, c):
        D = self.mod["D"]; B, Q, lens = self.d_rows; lens, needle = self._too_long(lens, B.shape[1])
        return self._on_rows(c, D.dev_rows(c, B, Q, lens), lambda d: self._refused((-3,), needle, lambda: D.run(c, d, pairs=True, best=True, hist_len=8)))

    def bad_profile_rows(self, c):
        """a window past the read in the last row: the call's own exit (PF_ERR_WIN), beside the family's bad length"""
        needle = "ends behind its read: start < 0, len < 0 or start + len > lens[i] (first such row: %d)" % (len(self.p_bad[2]) - 1)
        return self._refused((-3,), needle, lambda: self.profile_rows(c, rows=self.p_bad))

    def bad_screen_rows(self, c):
        lens, needle = self._too_long(self.s_rows[1], self.s_rows[0].shape[1])
        return self._refused((-3,), needle, lambda: self.screen_rows(c, lens=lens))      # (the build in front of it is a good one)

    def bad_kmers_rows(self, c):
        K, Sc = self.mod["K"], self.mod["Sc"]; B, lens = self.k_rows[0]; lens, needle = self._too_long(lens, B.shape[1])
        t = K.Table(c, self.k_k, K.pow2(2 * len(self.k_cnt)))
        try:
            return self._on_rows(c, Sc.dev_rows(c, B, lens), lambda d: self._refused((-3,), needle, lambda: t.count(d)))
        finally:
            t.free()

    def kmers_full(self, c):
        """the good rows into a table of the smallest size, which has fewer slots than they have values: refused behind the kernels, the table is discarded"""
        return self._refused((RFQ_E_NOSPACE,), "the table is too full", lambda: self.kmers_rows(c, slots=1024))

    def bad_demux_rows(self, c):
        lens, needle = self._too_long(self.x_rows[1], self.x_rows[0].shape[1])
        return self._refused((-3,), needle, lambda: self.demux_rows(c, lens=lens))

    def bad_group_rows(self, c):
        G = self.mod["G"]; B, Q, lens, names, _ = self.g_rows; kw = self.g_kw
        dev = G.dev_group(c, B, Q, lens, names, self.g_bad, kw["keep"], kw["start"], kw["length"])
        return self._on_rows(c, dev, lambda d: self._refused((-3,), "first such unit: %d)" % self.g_bad_unit,
                                                             lambda: c.group_rows(*d.args(), **G.kw_of(d, self.g_bins, True, False, 1))))

    def bad_rows_to_text(self, c):
        dev = self.mod["W"].DevRows(c, *self.code_rows)
        return self._on_rows(c, dev, lambda d: self._refused((-5,), None, lambda: c.rows_to_text(*d.args(), paired=self.paired, codes=True)))

    def bad_encode_rows(self, c):
        def call(d):
            c.clearHeader()
            c.encode_rows(*d.args(), paired=self.paired, codes=True, chunk_bases=self.cb)
        return self._on_rows(c, self.mod["W"].DevRows(c, *self.code_rows), lambda d: self._refused((-5,), None, lambda: call(d)))

    def bad_text_rows(self, c):
        return self._refused((-5,), None, lambda: self.mod["T"].call(c, self.junk, b"", O.SE, None, codes=True, extra="x16"))

    def bad_decode_rows(self, c):
        import _hostile
        return self._refused(set(_hostile.ALLOWED), None, lambda: c.decode_rows_bytes(self.mutant))

    def bad_decode_names(self, c):
        import _hostile
        return self._refused(set(_hostile.ALLOWED), None, lambda: c.decode_names_bytes(self.mutant))

    def bad_encode(self, c):
        return self._refused((RFQ_E_DATA,), self.coord_said, lambda: E.encode(c, self.coord_fq, b"", O.SE, self.cb), exact=True)

    def bad_decode(self, c):
        return self._refused((RFQ_E_DATA,), self.split_said, lambda: c.decode_bytes(self.se_want, split_pe=True), exact=True)


REFUSING_CALL_KINDS = ("bad_select_rows", "bad_judge_rows", "bad_adapter_rows", "bad_merge_rows", "bad_dedup_rows", "bad_rows_to_text", "bad_encode_rows",
                       "bad_text_rows", "bad_decode_rows", "bad_decode_names", "bad_encode", "bad_decode", "bad_profile_rows", "bad_screen_rows", "bad_kmers_rows",
                       "kmers_full", "bad_demux_rows", "bad_group_rows")
# the good kind each refusing kind is a mutation of; and the kinds without one, with the reason (tests/test_call_kinds.py: every kind is in one of the two)
REFUSING_KIND_OF = dict({k: k[4:] for k in REFUSING_CALL_KINDS if k.startswith("bad_")}, kmers_full="kmers_rows")
NO_REFUSING_KIND = (
    ("scan", "the encoder's front (index and cut) and nothing behind it: its one exit on the device, enc_cut, is qual_short_late's in the refusal circuits over the inputs"),
    ("first_diff", "compares two byte ranges: no verdict block, nothing the device can refuse"),
)


def calls_refusal_circuit():
    """(kinds, seq): the good kinds and the refusing ones, every ordered pair adjacent once but good -> good (euler(len(CALL_KINDS)) has those)"""
    g, r = len(CALL_KINDS), len(REFUSING_CALL_KINDS)
    seq = circuit(range(g + r), refusal_edges(g, r))
    assert len(seq) == 2 * g * r + r * r + 1, (g, r, len(seq))
    return CALL_KINDS + REFUSING_CALL_KINDS, seq


_CALLS = None


def calls():
    global _CALLS
    if _CALLS is None:
        _CALLS = Calls()
    return _CALLS


def first_results(make_codec):
    """{kind: what the call gives first on a fresh context} - each checked against its host reference inside the call"""
    out = {}
    for kind in CALL_KINDS:
        c = make_codec()
        try:
            if kind in CALL_STAGES:                                          # (the step reaches the stages it is there for)
                marks = set()
                out[kind] = getattr(calls(), kind)(c, marks=marks)
                assert set(CALL_STAGES[kind]) <= marks, (kind, CALL_STAGES[kind], sorted(marks))
            else:
                out[kind] = getattr(calls(), kind)(c)
        finally:
            c.close()
    return out


def walk_calls(codec, first, seq, start=0, stop=None, prev=None, kinds=CALL_KINDS):
    """kinds: what seq indexes; a refusing kind (not in `first`) is checked by its code and message alone"""
    from repaq_amd import RfqError
    stop = len(seq) if stop is None else stop
    bad = []
    for i in range(start, stop):
        kind = kinds[seq[i]]
        try:
            got = getattr(calls(), kind)(codec)
            if kind in first and got != first[kind]:
                bad.append("step %d: %s behind %s equals its reference but not its own first result" % (i, kind, prev or "a fresh context"))
        except (AssertionError, RfqError) as e:                              # (behind a refusing kind a good call may be refused: collected like a difference)
            bad.append("step %d: %s behind %s: %s" % (i, kind, prev or "a fresh context", str(e)[:300]))
        prev = kind
    assert not bad, "%d of %d calls differ:\n%s" % (len(bad), stop - start, "\n".join(bad[:12]))
    return prev


# ---------------------------------------------------------------- nothing is left of a larger call
# _dedup.check_state's pattern for the other rows calls, which share rfq_ctx::b[] scratch that only grows: a LARGE batch (5000 rows at a stride of 1100 bytes: the
# any-length kernels, the largest scratch), then a SMALL one (40 rows at a stride of 150, every one a row of the large batch) on the same context - the small one's
# bytes and summary are a fresh context's, and the large batch again gives its own first result.  Both sizes are compared with the module's host reference inside
# every call.  One row in 25 of the large batch is 1100 bases long, the others 100 .. 150: the host references are Python loops over the bases.
NOTHING_LEFT_CALLS = ("decode_rows", "decode_names", "text_rows", "select_rows", "judge_rows", "adapter_rows", "merge_rows", "rows_to_text", "encode_rows",
                      "dedup_rows", "profile_rows", "screen_rows", "kmers_rows", "demux_rows", "group_rows")
# the kinds that are not among them, with the reason (tests/test_call_kinds.py: every kind is in one of the two; every rows kind is above)
NO_NOTHING_LEFT = (
    ("encode", "the circuits over the inputs run three_records behind se150_big: buffers far larger than the batch"),
    ("decode", "the same circuits, decoding"),
    ("scan", "the encoder's front: the same buffers, the same circuits"),
    ("first_diff", "keeps one word of scratch whatever the size"),
)
BIG_ROWS, BIG_LEN, SMALL_ROWS, SMALL_LEN = 5000, 1100, 40, 150


def _embed(short, long_, L):
    """row arrays of two strides, one above the other at stride L (what lies behind a short row's own stride is padding: 255)"""
    out = np.full((len(short) + len(long_), L), 255, np.uint8)
    out[:len(short), :short.shape[1]] = short; out[len(short):, :long_.shape[1]] = long_
    return out


class Batch:
    """the inputs of the fifteen calls at one size, and their host references; small=True: rows that all occur in Batch(False)"""
    def __init__(self, small, mod):
        import _rows_enc as R
        A, J = mod["A"], mod["J"]
        self.mod, self.small = mod, small
        rng = np.random.default_rng(61); recs = []
        for i in range(BIG_ROWS):
            ln = BIG_LEN if i % 25 == 0 else (SMALL_LEN if i % 25 == 1 else int(rng.integers(100, SMALL_LEN + 1)))
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)]; seq[rng.random(ln) < 0.002] = ord("N")
            q = np.frombuffer(b"FFFFFF:,", np.uint8)[rng.integers(0, 8, ln)]; q[seq == ord("N")] = ord("#")
            recs.append(b"@A00250:26:H3YTWDSXX:1:%d:%d:%d 1:N:0:ACGT\n" % (1101 + i // 500, 1000 + 37 * i % 29000, 1000 + 11 * (i % 500)) + seq.tobytes() + b"\n+\n" + q.tobytes() + b"\n")
        if small:
            short = [i for i in range(BIG_ROWS) if i % 25]                    # (the first of them, record 1, is 150 bases long: the small batch's stride)
            recs = [recs[i] for i in short[::len(short) // SMALL_ROWS][:SMALL_ROWS]]
        self.L = SMALL_LEN if small else BIG_LEN
        self.fq = b"".join(recs); self.cb = 30000 if small else 1_000_000
        self.want = O.encode_file(self.fq, b"", O.SE, self.cb)
        assert O.decode_file(self.want) == self.fq
        self.rows = R.rows_of(self.fq, b"", O.SE)
        n = len(self.rows[2])
        assert self.rows[0].shape == (SMALL_ROWS if small else BIG_ROWS, self.L)
        self.sel = dict(keep=(rng.random(n) < 0.8).astype(np.uint8), start=rng.integers(0, 20, n).astype(np.int32), length=rng.integers(0, 80, n).astype(np.int32),
                        min_len=30)                                          # (windows within a read of 100 bases)
        self.j_crit = dict(J.STEPS)["all"]; self.a_crit = A.shape_criteria(SMALL_LEN)[2][1]

    # (every reference is made when its call is first checked, and once)
    @functools.cached_property
    def rows_want(self):
        e = self.mod["W"].expected(self.want)
        assert e[1] == self.L
        return e

    @functools.cached_property
    def names_want(self):
        return self.mod["N"].expected(self.want)

    @functools.cached_property
    def recs(self):
        return self.mod["T"].expect(self.fq, b"", O.SE, self.cb)[1]

    @functools.cached_property
    def j_want(self):
        B, Q, lens, _ = self.rows
        return self.mod["J"].expected(B, Q, lens, self.j_crit, False)

    # pairs: 2400 of rows of 150 bytes and 100 of rows of 1100; the small batch is the first 20 of the short ones
    @functools.cached_property
    def a_rows(self):
        A = self.mod["A"]
        sB, sl = A.random_pairs(2400, SMALL_LEN, 62, codes=True); lB, ll = A.random_pairs(100, BIG_LEN, 63, codes=True)
        rows = (sB[:SMALL_ROWS], sl[:SMALL_ROWS]) if self.small else (_embed(sB, lB, BIG_LEN), np.concatenate([sl, ll]))
        assert rows[0].shape == (SMALL_ROWS if self.small else BIG_ROWS, self.L)
        return rows

    @functools.cached_property
    def a_want(self):
        return self.mod["A"].expected(*self.a_rows, self.a_crit, True)

    @functools.cached_property
    def m_rows(self):
        M = self.mod["M"]
        sB, sQ, sl, sn, si = M.random_pairs(2400, SMALL_LEN, 64, codes=False); lB, lQ, ll, ln_, li = M.random_pairs(100, BIG_LEN, 65, codes=False)
        rows = ((sB[:SMALL_ROWS], sQ[:SMALL_ROWS], sl[:SMALL_ROWS], sn[:SMALL_ROWS], si[:SMALL_ROWS // 2]) if self.small else
                (_embed(sB, lB, BIG_LEN), _embed(sQ, lQ, BIG_LEN), np.concatenate([sl, ll]), list(sn) + list(ln_), np.concatenate([si, li])))
        assert rows[0].shape == (SMALL_ROWS if self.small else BIG_ROWS, self.L)
        return rows

    @functools.cached_property
    def m_want(self):
        return self.mod["M"].expected(*self.m_rows, False)

    # --- the six kinds behind encode_rows: the batch's own rows (5000 at a stride of 1100, 40 at 150), and per-call parameters that differ in the direction that
    # leaves something behind - the large call has the longer barcodes, the more bins, the larger k and table, the tables beyond the LDS
    @functools.cached_property
    def d_rows(self):
        """the rows with planted classes: six rows in ten take the bytes and the length of one of a few others (rows 0 and 1 among them: 1100 and 150 bases in
        the large batch), every row with scores of its own"""
        B, Q, lens, _ = self.rows; n = len(lens); rng = np.random.default_rng(66)
        pool = np.concatenate([[0, 1], rng.choice(np.arange(2, n), max(3, n // 100), replace=False)])
        src = np.arange(n); planted = rng.random(n) < 0.6
        src[planted] = pool[rng.integers(0, len(pool), int(planted.sum()))]
        return np.ascontiguousarray(B[src]), rng.integers(0, 42, Q.shape).astype(np.uint8), lens[src]

    @functools.cached_property
    def d_want(self):
        e = self.mod["D"].expected(*self.d_rows, best=True, hist_len=8)
        assert e["summary"]["max_class"] >= 5 and e["summary"]["n_dups"] > len(self.d_rows[2]) // 3
        return e

    @functools.cached_property
    def p_kw(self):
        return dict(pairs=False, cycles=7, qbins=3, len_bins=2) if self.small else dict(pairs=True, cycles=BIG_LEN, qbins=64, len_bins=BIG_LEN + 1)

    @functools.cached_property
    def p_want(self):
        B, Q, lens, _ = self.rows; kw = self.p_kw
        return self.mod["P"].expected(B, Q, lens, False, kw["pairs"], self.sel["keep"], self.sel["start"], self.sel["length"], kw["cycles"], kw["qbins"], kw["len_bins"])

    def _seq(self, i):
        return self.rows[0][i, :int(self.rows[2][i])].tobytes()

    @functools.cached_property
    def s_refs(self):
        """(references, k): the large batch k = 31 and forty of its rows whole (the first, of 1100 bases, among them); the small one k = 15 and two stretches
        of 120 bases of its rows - 240 bases: an index of the smallest size, 1024 slots"""
        n = len(self.rows[2])
        return ([self._seq(0)[15:135], self._seq(n // 2)[:120]], 15) if self.small else ([self._seq(i) for i in range(0, n, n // 40)], 31)

    @functools.cached_property
    def s_kw(self):
        return dict(pairs=not self.small, min_hits=2, min_pct=10)

    @functools.cached_property
    def s_want(self):
        Sc = self.mod["Sc"]; refs, k = self.s_refs
        self.s_set = Sc.ref_set(refs, k)[0]
        e = Sc.expected(self.rows[0], self.rows[2], self.s_set, k, False, **self.s_kw)
        assert 0 < e["summary"]["n_matched"] < e["summary"]["n_candidates"]
        return e

    @functools.cached_property
    def k_want(self):
        """(k, slots, cand, the model's Counter, kmers, summary): the large batch k = 31 in a table of twice its values; the small one k = 15 and its first three
        rows, which is what the smallest table (1024 slots, for 512 values) takes"""
        K = self.mod["K"]; B, _, lens, _ = self.rows
        k = 15 if self.small else 31
        cand = (np.arange(len(lens)) < 3).astype(np.uint8) if self.small else None
        cnt, kmers, s = K.model(B, lens, k, False, cand)
        slots = K.pow2(2 * len(cnt))
        assert (slots == 1024 and 256 < len(cnt) <= 512) if self.small else slots >= 1 << 18, (slots, len(cnt))
        return k, slots, cand, cnt, kmers, dict(s, n_new=len(cnt), n_kmers=len(cnt), total=sum(cnt.values()), lost=0)

    @functools.cached_property
    def x_case(self):
        """(B, lens, Cfg): the large batch as pairs against two sets of 512 barcodes of 32 bases, every combination a sample (262144 count cells: beyond the LDS
        table); the small one as rows against one set of 3 barcodes of 8.  The barcodes are planted into a copy of the rows - exact, with one and with three
        mismatches, from a pool of a few hundred windows, so that the model's loop over the barcodes runs once per window -; one row in 50 keeps its own bases"""
        X = self.mod["X"]; B, _, lens, _ = self.rows; B = B.copy(); n = len(lens); rng = np.random.default_rng(67)
        if self.small:
            sets = [X.distinct_barcodes(rng, 3, 8, min_dist=3)]; cfg = X.Cfg(sets[0], off1=3, skip1=2)
        else:
            sets = [[X.rand_seq(rng, 32) for _ in range(512)] for _ in range(2)]      # (random 32-mers: about 24 bases apart)
            assert all(len(set(x)) == 512 for x in sets)
            cfg = X.Cfg(sets[0], sets[1], pairs=True, off1=3, off2=0, skip1=2, skip2=1, max_mm=1, min_delta=1)
        for m, bcs in enumerate(sets):
            pool = []
            for j in range(0, len(bcs), max(1, len(bcs) // 64)):
                b = bcs[j]; pool += [b, X.mutate(b, j % len(b)), X.mutate(X.mutate(X.mutate(b, 0), 3), 5), X.mutate(b, 1, ord("N"))]
            pool = np.array([np.frombuffer(p, np.uint8) for p in pool])
            rows = np.arange(m, n, len(sets)); rows = rows[rows % 50 >= 2]
            off = cfg.off[m]
            B[rows, off:off + pool.shape[1]] = pool[rng.integers(0, len(pool), len(rows))]
        return B, lens, cfg

    @functools.cached_property
    def x_want(self):
        B, lens, cfg = self.x_case
        e = self.mod["X"].expected(B, lens, cfg, False); s = e["summary"]
        assert s["n_assigned"] > s["n_units"] // 4 and s["why_none"] > 0 and s["n_exact"] < s["n_assigned"], s
        return e

    @functools.cached_property
    def g_case(self):
        """(bins, n_bins, rest): the large batch over 4097 bins, all of them in reach, and the rest bin; the small one over 3 bins, and units of bin -1 fall"""
        n = len(self.rows[2]); rng = np.random.default_rng(68)
        if self.small:
            return (np.arange(n) % 4 - 1).astype(np.int32), 3, False
        bins = rng.integers(-1, 4097, n).astype(np.int32); bins[:3] = (4096, 0, -1)
        return bins, 4097, True

    def dedup_rows(self, c):
        D = self.mod["D"]; dev = D.dev_rows(c, *self.d_rows)
        try:
            out, summ, raw = D.run(c, dev, best=True, hist_len=8)
        finally:
            dev.free()
        D.compare(out, summ, self.d_want, "nothing left:")
        return _items(raw), _items(summ)

    def profile_rows(self, c):
        P = self.mod["P"]; B, Q, lens, _ = self.rows
        dev = P.dev_rows(c, B, Q, lens, self.sel["keep"], self.sel["start"], self.sel["length"])
        try:
            out, summ, raw = P.run(c, dev, False, **self.p_kw)
        finally:
            dev.free()
        P.compare(out, summ, self.p_want, "nothing left:")
        return _items(raw), _items(summ)

    def screen_rows(self, c):
        Sc = self.mod["Sc"]; want = self.s_want; refs, k = self.s_refs
        idx = Sc.Index(c, refs, k)
        try:
            assert (idx.bytes == 64 + 8 * 1024) == self.small
            index = _index_set(idx.g.body())
            assert index[1] == _slots_of(self.s_set), "nothing left: the index is not the model's set"
            dev = Sc.dev_rows(c, self.rows[0], self.rows[2])
            try:
                out, summ, raw = Sc.run(c, dev, idx, **self.s_kw)
            finally:
                dev.free()
        finally:
            idx.free()
        Sc.compare(out, summ, want, "nothing left:")
        return index, _items(raw), _items(summ)

    def kmers_rows(self, c):
        K, Sc = self.mod["K"], self.mod["Sc"]; k, slots, cand, cnt, kmers, want = self.k_want
        t = K.Table(c, k, slots)
        try:
            dev = Sc.dev_rows(c, self.rows[0], self.rows[2], cand)
            try:
                got, summ, raw = t.count(dev)
            finally:
                dev.free()
            assert np.array_equal(got, kmers), "nothing left: kmers differ, first in row %d" % int(np.nonzero(got != kmers)[0][0])
            assert summ == want, ("nothing left:", {f: (summ[f], want[f]) for f in K.ROWS_FIELDS if summ[f] != want[f]})
            read = t.check(hist_len=16, cnt=cnt, what="nothing left")
            return raw, _items(summ), tuple(read["pairs"]), read["hist"].tobytes(), _items(read["summary"])
        finally:
            t.free()

    def demux_rows(self, c):
        X = self.mod["X"]; B, lens, cfg = self.x_case; want = self.x_want
        dev = X.dev_rows(c, B, lens)
        try:
            out, summ, raw = X.run(c, dev, cfg, False, X.ALL)
        finally:
            dev.free()
        X.compare(out, summ, want, "nothing left:")
        return _items(raw), _items(summ)

    def group_rows(self, c):
        G = self.mod["G"]; B, Q, lens, names = self.rows; bins, n_bins, rest = self.g_case
        e, r, got = G.call(c, B, Q, lens, names, bins, n_bins, rest=rest, keep=self.sel["keep"], start=self.sel["start"], length=self.sel["length"],
                           min_len=self.sel["min_len"], per_bin=False)
        assert (r.n_bins_used > 1000 and r.dropped_bin == 0) if rest else (r.n_bins_used == 3 and r.dropped_bin > 0), (r.n_bins_used, r.dropped_bin)
        return G.fields_of(r), _items(got)

    def decode_rows(self, c):
        n, ml, B, Q, lens = self.rows_want
        gn, gml, gb, gq, gl = c.decode_rows_bytes(self.want)
        assert (gn, gml) == (n, ml) and np.array_equal(gl, lens) and np.array_equal(gb, B) and np.array_equal(gq, Q), "decode_rows differs from the host's rows"
        return gn, gml, gb.tobytes(), gq.tobytes(), gl.tobytes()

    def decode_names(self, c):
        return tuple(self.mod["N"].check(c, self.want, want=self.names_want))

    def text_rows(self, c):
        r, B, Q, lens, names = self.mod["T"].call(c, self.fq, b"", O.SE, recs=self.recs)
        return (int(r.n_rows), int(r.consumed1), int(r.max_len)), B.tobytes(), Q.tobytes(), lens.tobytes(), tuple(names)

    def select_rows(self, c):
        r = self.mod["S"].call(c, *self.rows, **self.sel)
        return (int(r[0].n_rows), int(r[0].n_bases), int(r[0].dropped_mask), int(r[0].dropped_short)), tuple(r[5])

    def judge_rows(self, c):
        J, W = self.mod["J"], self.mod["W"]; B, Q, lens, _ = self.rows; dev = W.DevRows(c, B, Q, lens)
        try:
            out, summ, raw = J.run(c, dev, self.j_crit, False)
        finally:
            dev.free()
        J.compare(out, summ, self.j_want, "nothing left:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def adapter_rows(self, c):
        A, W = self.mod["A"], self.mod["W"]; B, lens = self.a_rows; dev = W.DevRows(c, B, None, lens)
        try:
            out, summ, raw = A.run(c, dev, self.a_crit, True)
        finally:
            dev.free()
        A.compare(out, summ, self.a_want, "nothing left:")
        return tuple(sorted(raw.items())), tuple(sorted(summ.items()))

    def merge_rows(self, c):
        e, _, _, raw = self.mod["M"].call(c, *self.m_rows, False, paths=(None,), e=self.m_want)
        return len(e["idx"]), tuple(raw)

    def rows_to_text(self, c):
        got = c.rows_to_text_bytes(*self.rows)
        assert got == self.fq, text_diff(got, self.fq)
        return got

    def encode_rows(self, c):
        c.clearHeader()
        got = c.encode_rows_bytes(*self.rows, chunk_bases=self.cb, **E.nolb_args(self.fq, b"", O.SE))
        assert got == self.want, image_diff(got, self.want)
        return got


_BATCHES = {}


def batch(small):
    if small not in _BATCHES:
        _BATCHES[small] = Batch(small, calls().mod)
    return _BATCHES[small]


def check_nothing_left(codec, make_codec, kind):
    """one context: the large batch, the small one, the large one again - see above"""
    big, small = batch(False), batch(True)
    fresh = make_codec()
    try:
        want = getattr(small, kind)(fresh)
    finally:
        fresh.close()
    first = getattr(big, kind)(codec)
    got = getattr(small, kind)(codec)
    assert got == want, "%s: a small batch behind a large one equals its reference but not a fresh context's result" % kind
    again = getattr(big, kind)(codec)
    assert again == first, "%s: the large batch again equals its reference but not its own first result" % kind


# ---------------------------------------------------------------- state whose loss costs time, not bytes
def check_mixed_lengths_end_with_the_file(make_codec):
    """rfq_ctx::mixed_lengths (the prefix scans up front, no index without a read-back) is reset by new_file(): a uniform file encoded behind a file of mixed lengths
    is indexed without the read-back again.  A bit that stays up gives the same bytes by the slower route - no circuit can see it, the `lazy_index` stage can."""
    c = make_codec()
    try:
        for name in ("se150_big", "se_var", "se150_big", "three_records", "se150_big"):
            inp = by_name(name)
            msg = encode_step(c, inp)
            assert not msg, (name, msg)
            marks = {n for n, _ in c.timings()}
        assert "lazy_index" in marks, sorted(marks)
    finally:
        c.close()
