"""Shared helpers of the rfq_decode_names tests (tests/test_emu_names.py on the SIMT interpreter, tests/test_gpu_names.py on the MI355X).

The expected names never come from the kernel: the plain-C oracle decodes the image to text (_oracle.decode_file(rfq, False): Repaq::decompress
order), the text is split on '\\n' and every fourth line is a name."""
import ctypes as C
import time

import numpy as np

import _engine as E
import _hostile as H
import _oracle as O
import _rows as W
import _rows_enc as R


def expected(rfq: bytes, text=None):
    """the name lines of the oracle's text of the image ('@' included, no line breaks)"""
    return (O.decode_file(rfq, False) if text is None else text).split(b"\n")[:-1][0::4]


def offsets(names):
    off = np.zeros(len(names) + 1, np.uint64)
    if names:
        off[1:] = np.cumsum([len(x) for x in names])
    return off


def fetch(codec, r):
    """(names, offsets) of a DecodeNamesResult"""
    n = int(r.n_rows)
    off = np.frombuffer(codec.dev_get(r.d_name_off, 8 * (n + 1)), np.uint64)
    blob = codec.dev_get(r.d_names, int(r.names_len)) if r.names_len else b""
    return [blob[int(off[i]):int(off[i + 1])] for i in range(n)], off


def check(codec, rfq: bytes, want=None, **kw):
    """rfq_decode_names on the image: names, offsets, n_rows, names_len, max_name and consumed against the oracle's text; returns the names"""
    want = expected(rfq) if want is None else want
    d = codec.dev_put(rfq)
    try:
        r = codec.decode_names(d, len(rfq), **kw)
        got, off = fetch(codec, r)
    finally:
        codec.dev_free(d)
    assert r.n_rows == len(want), (r.n_rows, len(want))
    assert np.array_equal(off, offsets(want)), "offsets differ"
    assert r.names_len == sum(len(x) for x in want) and r.max_name == max([len(x) for x in want] + [0]), (r.names_len, r.max_name)
    assert r.consumed == len(rfq), (r.consumed, len(rfq))
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert not bad, "names differ from the oracle: %d of %d, first %d: %r / %r" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])
    return got


def check_size_only(codec, rfq: bytes, **kw):
    """the size query alone: the counts of check(), no pointers, and of the stages the lengths but not the writer"""
    want = expected(rfq)
    d = codec.dev_put(rfq)
    try:
        q = codec.decode_names(d, len(rfq), size_only=True, **kw)
    finally:
        codec.dev_free(d)
    assert (q.n_rows, q.names_len, q.max_name, q.consumed) == (len(want), sum(len(x) for x in want), max([len(x) for x in want] + [0]), len(rfq))
    assert q.d_names is None and q.d_name_off is None
    stages = dict(codec.timings())
    assert {"walk", "name_lens"} <= set(stages) and "names" not in stages, stages


# ---------------------------------------------------------------- small shapes where the writer can go wrong
def _image(text, text2=b"", paired=O.SE, chunk_bases=8000, min_chunks=3):
    rfq = O.encode_file(text, text2, paired, chunk_bases)
    assert len(O.chunk_table(rfq)) - 1 >= min_chunks
    return rfq


def unparsed_names():
    """(a) 600 SE reads under names FastqMeta::parse does not take apart, of 2..255 bytes ('@' included): the first 300 short (tiles composed in LDS), then
    every length up to 255 (tiles of more bytes than the LDS tile holds: byte-wise).  The names start at every residue mod 16 (asserted)."""
    def name_of(i):
        k = 1 + (i * 7) % 39 if i < 300 else 1 + (i * 37) % 254
        return "".join(chr(97 + (i + 3 * j) % 26) for j in range(k))
    text = E.handmade(600, name_of, lambda i: 50, lambda i: "+", seed=31)
    names = R.lines_of(text)[0::4]
    assert {len(x) for x in names} >= set(range(2, 256)) and {int(o) % 16 for o in offsets(names)[:-1]} == set(range(16))
    return _image(text), names


COORDS = (0, 9, 10, 99, 100, 99999, 100000, 999999, 1000000, 2097151)       # (2^21 - 1: the largest value the coordinate coder stores)


def illumina_digit_counts():
    """(b) sequencer names whose lane / tile / x / y cross every digit count the format can hold: lane up to 255, tile up to 65535, x / y up to 2^21 - 1"""
    def name_of(i):
        return "M0:7:FC:%d:%d:%d:%d 1:N:0:ACGT" % ((1, 9, 10, 99, 100, 255)[i % 6], (0, 9, 10, 999, 1101, 10000, 65535)[i % 7], COORDS[i % 10], COORDS[(i // 10) % 10])
    text = E.handmade(420, name_of, lambda i: 60, lambda i: "+", seed=32)
    return _image(text), R.lines_of(text)[0::4]


def coordinates_beyond_the_format():
    """x / y of 99999999 and of 10^8 and more (mid_put's loop path) cannot be stored: the coordinate coder takes values below 2^21 and the reference
    refuses the file (src/rfqcodec.cpp: "The X/Y coordinate cannot be larger than 2M").  Returns the oracle's refusals."""
    out = []
    for v in (99999999, 100000000, 4294967295):
        text = E.handmade(4, lambda i: "M0:7:FC:1:1101:%d:5 1:N:0:ACGT" % v, lambda i: 30, lambda i: "+", seed=33)
        try:
            O.encode_file(text, b"", O.SE, 1000)
            out.append(None)
        except O.OracleError as e:
            out.append(str(e))
    return out


def pe_pair(n=240, differ=True, per_read_name2=False, seed=34):
    """(c) two texts whose mates differ in one name2 character ("1:N:0" / "2:N:0") or not at all; per_read_name2: an index that changes from pair to pair"""
    def two(k):
        def name_of(i):
            tail = "%d:N:0:%s" % (k if differ else 1, ("ACGT" + "ACGT"[i % 4] * (i % 5)) if per_read_name2 else "ACGT")
            return "A00250:26:H3YTWDSXX:1:1101:%d:%d %s" % (1000 + i, 2000 + i // 7, tail)
        return E.handmade(n, name_of, lambda i: 70, lambda i: "+", seed=seed + k)
    return two(1), two(2)


def interleave(fq1, fq2):
    l1, l2 = R.lines_of(fq1), R.lines_of(fq2)
    return b"".join(b"\n".join(l[i:i + 4]) + b"\n" for i in range(0, len(l1), 4) for l in (l1, l2))


def pe_shapes():
    out = []
    for differ, per_read in ((True, False), (False, False), (True, True)):
        a, b = pe_pair(differ=differ, per_read_name2=per_read)
        tag = ("differ" if differ else "same") + ("_per_read_name2" if per_read else "")
        out.append(("two_files_" + tag, _image(a, b, O.PE_TWO_FILES, 9000)))
        out.append(("interleaved_" + tag, _image(interleave(a, b), b"", O.PE_INTERLEAVED, 9000)))
    return out


def tiny_shapes():
    """(d) one read in one chunk; one read per chunk"""
    one = E.handmade(1, lambda i: "A00250:26:H3YTWDSXX:1:1101:1000:2000 1:N:0:ACGT", lambda i: 40, lambda i: "+", seed=35)
    five = E.handmade(5, lambda i: "A00250:26:H3YTWDSXX:1:1101:%d:2000 1:N:0:ACGT" % (1000 + 7 * i), lambda i: 40, lambda i: "+", seed=36)
    return [("one_read", _image(one, chunk_bases=1000, min_chunks=1)), ("one_read_per_chunk", _image(five, chunk_bases=1, min_chunks=5))]


def write_fixtures(directory):
    """two images for the stand-alone sanitizer program (tools/names_asan.sh): per-read names past the LDS tile, and interleaved mates with a per-read name2"""
    import os
    out = []
    for label, rfq in (("unparsed", unparsed_names()[0]), ("interleaved_per_read_name2", dict(pe_shapes())["interleaved_differ_per_read_name2"])):
        path = os.path.join(directory, label + ".rfq")
        with open(path, "wb") as f:
            f.write(rfq)
        out.append(path)
    return out


# ---------------------------------------------------------------- the streaming contract
def decode_names_in_slices(codec, rfq: bytes, step: int):
    """`step` bytes at a time (has_header on the first call, final on the last, the unconsumed tail carried over); size_only must agree with the decode"""
    out = []
    pos, end, first = 0, min(step, len(rfq)), True
    while True:
        final = end == len(rfq)
        buf = rfq[pos:end]
        d = codec.dev_put(buf)
        try:
            q = codec.decode_names(d, len(buf), size_only=True, has_header=first, final=final)
            r = codec.decode_names(d, len(buf), has_header=first, final=final)
            assert (r.n_rows, r.consumed, r.names_len, r.n_chunks) == (q.n_rows, q.consumed, q.names_len, q.n_chunks)
            out += fetch(codec, r)[0]
            consumed = r.consumed
        finally:
            codec.dev_free(d)
        first = False
        if final:
            break
        pos += consumed
        end = min(len(rfq), max(end, pos) + step)
    return out


# ---------------------------------------------------------------- the loop closes
def reencodes(label):
    """the filter of _rows_enc.check_image's second leg, from the oracle alone: the image holds the text's reads whole, every strand line is "+" - and
    the image holds the text's NAMES (check_image feeds the text's names back; here they come out of the image, and the format does not keep every
    name: FastqMeta::parse's quirks turn "@A:B:C:D:E rest" into "@A:B:C:D:0:0:0:0 rest", a file that mixes sequencer and other names loses the
    coordinates - such an image cannot come back from what it holds)"""
    _, fq1, fq2, paired, cb = R.BY_LABEL[label]
    want = O.encode_file(fq1, fq2, paired, cb)
    B, Q, lens, names = R.rows_of(fq1, fq2, paired)
    on, _, oB, oQ, ol = W.expected(want)
    whole = on == len(names) and np.array_equal(ol, lens) and np.array_equal(oB, B) and np.array_equal(oQ, Q)
    plus = all(R.lines_of(t)[2::4] == [b"+"] * (len(R.lines_of(t)) // 4) for t in (fq1, fq2) if t)
    kept = expected(want) == names
    return whole and plus and kept, want


def check_loop(codec, label):
    """the rows of rfq_decode_rows + the DEVICE names of rfq_decode_names, handed to rfq_encode_rows as device pointers, give the oracle's image"""
    ok, want = reencodes(label)
    if not ok:
        return False
    _, fq1, fq2, paired, cb = R.BY_LABEL[label]
    n, ml, gb, gq, gl = codec.decode_rows_bytes(want)
    ptrs = [codec.dev_put(x.tobytes()) for x in (gb, gq, gl)]
    d = codec.dev_put(want)
    try:
        r = codec.decode_names(d, len(want))
        assert r.n_rows == n
        codec.clearHeader()
        e = codec.encode_rows(n, gb.shape[1], ptrs[0], ptrs[1], ptrs[2], r.d_names, r.names_len, r.d_name_off, paired=paired, chunk_bases=cb,
                              **E.nolb_args(fq1, fq2, paired))
        again = codec.dev_get(e.d_rfq, e.rfq_len)
    finally:
        codec.dev_free(d)
        for p in ptrs:
            codec.dev_free(p)
    assert again == want, (label, len(again), len(want))
    return True


# ---------------------------------------------------------------- hostile images
def run_hostile(codec, modes=((),), counts=None, seed=7, time_bound_s=60.0, good_every=1, tame=False):
    """_hostile's images and mutants through rfq_decode_names, as _rows.run_hostile does for rows: every call returns one of _hostile.ALLOWED or names
    within the time bound, and after every `good_every`-th mutant the same context decodes the good image to the right names.  Names go into buffers sized
    for the good image (a mutant that claims more gets RFQ_E_NOSPACE).  Returns a summary dict."""
    from repaq_amd import RfqError
    summary = {"mutants": 0, "errors": {}, "decoded": 0, "slowest_s": 0.0, "slowest": None, "good_checks": 0}
    for label, img, _split, _want in H.images():
        want = expected(img); woff = offsets(want); n = len(want); nb = int(woff[-1])
        muts = H.mutants(img, seed, counts, tame)
        for mode in modes:
            for name, value in mode:
                codec.set_option(name, value)
            ob, oo = codec.dev_put(b"\0" * nb), codec.dev_put(b"\0" * (8 * (n + 1)))
            full = dict(d_names=ob, names_cap=nb, d_name_off=oo, off_cap=n + 1)
            try:
                for k, (mlabel, mimg, index) in enumerate(muts):
                    t0 = time.perf_counter()
                    d = codec.dev_put(mimg)
                    try:
                        codec.decode_names(d, len(mimg), **full, **({"chunk_off": index} if index else {}))
                        summary["decoded"] += 1; what = "decoded"
                    except RfqError as e:
                        oom = e.code == -2 and "out of memory" in e.message.lower()
                        assert e.code in H.ALLOWED or oom, "%s / %s / %s: error code %d (%s)" % (label, mode, mlabel, e.code, e.message)
                        what = "OOM" if oom else H.ALLOWED[e.code]
                        summary["errors"][what] = summary["errors"].get(what, 0) + 1
                    finally:
                        codec.dev_free(d)
                    dt = time.perf_counter() - t0
                    if dt > summary["slowest_s"]:
                        summary["slowest_s"], summary["slowest"] = round(dt, 3), "%s/%s" % (label, mlabel)
                    assert dt < time_bound_s, "%s / %s / %s took %.1f s" % (label, mode, mlabel, dt)
                    summary["mutants"] += 1
                    if k % good_every == 0 or k == len(muts) - 1:
                        d = codec.dev_put(img)
                        try:
                            r = codec.decode_names(d, len(img), **full)
                            got, off = fetch(codec, r)
                        finally:
                            codec.dev_free(d)
                        assert got == want and np.array_equal(off, woff), "%s / %s: the good image decodes to other names after mutant %s" % (label, mode, mlabel)
                        summary["good_checks"] += 1
            finally:
                codec.dev_free(ob); codec.dev_free(oo)
                for name, _ in mode:
                    codec.set_option(name, None)
    return summary


# ---------------------------------------------------------------- the tests themselves (the two files differ in the library and in the hostile counts)
def check_sizes_and_refusals(codec):
    """size_only == the decode's counts; guarded buffers of exactly names_len bytes (shift: a blob that starts one byte off) and n_rows + 1 entries;
    one byte / one entry short: -8, "need", nothing written, the next call right; a misaligned d_name_off: -3"""
    from repaq_amd import RfqError
    rfq = W.generated("pe150"); want = expected(rfq); woff = offsets(want); n = len(want); nb = int(woff[-1])
    d = codec.dev_put(rfq)
    try:
        q = codec.decode_names(d, len(rfq), size_only=True)
        assert (q.n_rows, q.names_len, q.max_name, q.consumed, q.n_chunks) == (n, nb, max(len(x) for x in want), len(rfq), len(O.chunk_table(rfq)) - 1)
        assert q.d_names is None and q.d_name_off is None
        qr = codec.decode_rows(d, len(rfq))
        assert (q.n_rows, q.n_chunks, q.consumed) == (qr.n_rows, qr.n_chunks, qr.consumed)
        for shift in (0, 1):
            gn, go = W.Guarded(codec, nb, shift=shift), W.Guarded(codec, 8 * (n + 1))
            try:
                assert go.ptr.value % 8 == 0 and gn.ptr.value % 16 == shift
                before = (gn.body(), go.body())
                for what, kw in (("blob one byte short", dict(names_cap=nb - 1, off_cap=n + 1)), ("offsets one entry short", dict(names_cap=nb, off_cap=n))):
                    with R.pytest_raises(RfqError) as ei:
                        codec.decode_names(d, len(rfq), d_names=gn.ptr, d_name_off=go.ptr, **kw)
                    assert ei.value.code == -8 and "need" in ei.value.message, (what, ei.value)
                    assert (gn.body(), go.body()) == before and gn.guards_intact() and go.guards_intact(), what
                r = codec.decode_names(d, len(rfq), d_names=gn.ptr, names_cap=nb, d_name_off=go.ptr, off_cap=n + 1)
                assert (r.n_rows, r.names_len, r.d_names, r.d_name_off) == (n, nb, gn.ptr.value, go.ptr.value)
                assert gn.body() == b"".join(want) and np.array_equal(np.frombuffer(go.body(), np.uint64), woff)
                assert gn.guards_intact() and go.guards_intact()
                with R.pytest_raises(RfqError) as ei:
                    codec.decode_names(d, len(rfq), d_names=gn.ptr, names_cap=nb, d_name_off=C.c_void_p(go.ptr.value + 4), off_cap=n + 1)
                assert ei.value.code == -3, ei.value
                assert gn.guards_intact() and go.guards_intact()
            finally:
                gn.free(); go.free()
        assert fetch(codec, codec.decode_names(d, len(rfq)))[0] == want
    finally:
        codec.dev_free(d)
