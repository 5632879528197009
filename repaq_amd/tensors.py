"""Decoded reads as torch tensors on the GPU (rfq_decode_rows): what a model, a k-mer counter or a quality filter takes.

    from repaq_amd import RfqCodec
    from repaq_amd.tensors import decode_tensors
    codec = RfqCodec(device=0)
    rfq = torch.from_file("x.rfq", size=n, dtype=torch.uint8).cuda()
    t = decode_tensors(codec, rfq)            # {"bases": [n, L] uint8 codes A0 C1 G2 T3 N4, "quals": [n, L] Phred, "lens": [n] int32}

and back - reads a basecaller, a simulator, a filter or a trimmer holds as tensors, straight to an image (rfq_encode_rows) or to FASTQ text:

    blob, off = pack_names([b"@r1", b"@r2"], device)
    image = encode_tensors(codec, t["bases"], t["quals"], t["lens"], blob, off)      # uint8 tensor: the .rfq image
    text = rows_to_fastq(codec, t["bases"], t["quals"], t["lens"], blob, off)        # uint8 tensor: the FASTQ text

decode -> filter / trim -> encode, three calls and nothing on the host (rfq_decode_names gives the names in pack_names' layout, rfq_select_rows compacts rows,
lengths, names and offsets in one pass):

    t = decode_tensors(codec, rfq, names=True)                                        # + "names": uint8 blob, "name_off": [n + 1] int64
    s = select_rows(codec, t, keep=t["lens"] >= 100, pairs=True)                      # any mask over the rows; a pair stands or falls together
    image = encode_tensors(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES)

fastq -> trim -> encode, the same without an image in front (rfq_text_rows: the text's own bytes, nothing an image would lose is lost); a window per row
keeps bases [start, start + length) of it, a read trimmed below min_len is dropped:

    fq = torch.from_file("x.fastq", size=n, dtype=torch.uint8).cuda()
    t = fastq_to_tensors(codec, fq)                                                   # "bases", "quals", "lens", "names", "name_off", "consumed"
    s = select_rows(codec, t, start=torch.full_like(t["lens"], 5), length=t["lens"] - 10, min_len=30)

fastq -> judge -> select -> encode, four calls and nothing on the host: rfq_judge_rows looks at the bases and the scores - it trims by quality (a sliding window
from either end), cuts poly-G tails, counts N, low scores and base changes - and leaves the keep mask and the window per row that select_rows takes, with a QC
summary of the batch (reads, bases, Q20 / Q30 before and after, rows per reason); filter_rows is the two in one:

    t = fastq_to_tensors(codec, fq1, fq2, paired=PE_TWO_FILES)
    j = judge_rows(codec, t, cut_tail=True, cut_window=4, cut_mean_q=20, poly_g=10, max_n=5, min_mean_q=20, qual_q=15, max_lowq_pct=40)
    s = select_rows(codec, t, keep=j["keep"], start=j["start"], length=j["length"], pairs=True, min_len=36)       # or: s = filter_rows(codec, t, pairs=True, min_len=36, ...)
    image = encode_tensors(codec, s["bases"], s["quals"], s["lens"], s["names"], s["name_off"], paired=PE_TWO_FILES)

adapter -> judge -> select: rfq_adapter_rows cuts adapters first - a pair whose insert is shorter than its reads is found by the overlap of R1 with the reverse
complement of R2, a known adapter sequence by a match at every position - and leaves the shortened lengths; the judge then trims and filters what is left, and
select_rows moves the bytes once:

    a = trim_adapters(codec, t, pairs=True, adapter1=b"AGATCGGAAGAGC", adapter2=b"AGATCGGAAGAGC")
    j = judge_rows(codec, dict(t, lens=a["length"]), cut_tail=True, cut_window=4, cut_mean_q=20, min_mean_q=20)
    s = select_rows(codec, t, keep=j["keep"], start=j["start"], length=j["length"], pairs=True, min_len=36)

adapter -> merge: the insert size trim_adapters finds for a pair is the length of the fragment both mates were read from; rfq_merge_rows collapses every such pair
into one read of that length - R1 from the front, the reverse complement of R2 from the back, a consensus by the scores where they overlap - under R1's name, and
the pairs without an overlap come back as they are:

    a = trim_adapters(codec, t, pairs=True); m = merge_pairs(codec, t, a["insert"])
    image = encode_tensors(codec, *(m["merged"][k] for k in ("bases", "quals", "lens", "names", "name_off")))          # SE; m["unmerged"]: the other pairs, PE

judge -> dedup -> select: rfq_dedup_rows relates the rows to each other - of every class of reads (or pairs) with identical bases it keeps one, the first or the
one with the best scores - and leaves the keep mask select_rows takes.  The judge's mask goes in as `keep`, so that a read that fails does not stand in for its
passing copies; the windows are still the judge's:

    j = judge_rows(codec, t, cut_tail=True, cut_window=4, cut_mean_q=20, min_mean_q=20)
    d = dedup_rows(codec, dict(t, lens=j["length"]), pairs=True, keep=j["keep"], best_qual=True)      # d["summary"]["n_dups"]: the duplication count of a QC report
    s = select_rows(codec, t, keep=d["keep"], start=j["start"], length=j["length"], pairs=True, min_len=36)

the report: rfq_profile_rows tabulates the rows under the same triple select_rows takes - base content and mean score per cycle, the position x score
distribution, the distributions of length, mean score and GC content, read 1 and read 2 apart - without moving a byte.  One call on the raw rows is the profile
"before filtering", one with the triple the profile "after filtering":

    before = profile_rows(codec, t, pairs=True)
    after = profile_rows(codec, t, pairs=True, keep=d["keep"], start=j["start"], length=j["length"])          # after["base_cnt"]: [2, cycles, 5] int64 ...

judge -> screen -> dedup -> select: rfq_screen_rows asks what a read IS - it counts, per read, the k-mers that occur in a set of reference sequences (the PhiX
spike-in, rRNA, a host, a bait set) and leaves the keep mask the next step takes; the set is built once, on the GPU, and is the caller's tensor:

    phix = screen_index(codec, [open("phix.fa").read().split("\n", 1)[1].replace("\n", "")], k=25)
    c = screen_rows(codec, dict(t, lens=j["length"]), phix, pairs=True, keep=j["keep"])                  # c["summary"]["n_matched"]: the spike-in's pairs
    d = dedup_rows(codec, dict(t, lens=j["length"]), pairs=True, keep=c["keep"])

the k-mers themselves: rfq_kmers_rows counts WHICH k-mers the reads hold, and how often, into a table that is the caller's tensor and adds up across the batches of
a file; its reader gives the spectrum, the (value, count) pairs and a screen index of the values in a count range - screening by abundance:

    tab = kmer_table(codec, k=25, slots=1 << 28)                                                        # >= 2 x the distinct k-mers expected
    count_kmers(codec, dict(t, lens=j["length"]), tab, keep=j["keep"])                                  # per batch, in any order
    kc = kmer_counts(codec, tab, min_count=2, hist_len=256, index=True)                                 # kc["hist"]: the spectrum; kc["values"], kc["counts"]: sorted by value
    c = screen_rows(codec, t, kc["index"], pairs=True, keep_matched=True, min_pct=50)                   # the pairs at least half made of k-mers seen twice

in front of all of these, a pooled run: rfq_demux_rows says WHOSE a read is - it compares the inline barcode at the front of R1 (and R2) with the sample sheet's
and leaves the sample per pair, the keep byte and the start select_rows takes, and the count per sample; one select_rows pass per sample splits the batch:

    dm = demux_rows(codec, t, i7, i5, sheet=[(0, 0), (1, 1), ...], pairs=True, skip1=1)                  # dm["counts"], dm["summary"]["why_combo"]: index hopping
    per_sample = split_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True)           # the unassigned rows last, whole

or, in ONE pass over the rows (rfq_group_rows: a stable sort of the kept units by bin; the bins are views of one result):

    g = group_rows(codec, t, dm["sample"], len(sheet), start=dm["start"], pairs=True)                    # g["bin_off"]: the first row of every bin
    per_sample = group_parts(g)                                                                          # one read-back; None for an empty bin

inline UMIs: the molecular barcode leaves the read and goes into its name while select_rows writes the name blob (rfq_name_tag) - fastp's --umi:

    s = extract_umi(codec, t, "per_read", 8, umi_skip=2, prefix="UMI", pairs=True)                       # names "@...:UMI_ACGTACGT_TTGCAAGG 1:N:0:ACGT"; start=dm["start"]: behind a barcode

A torch mask still works (t["bases"][keep] and so on), but the name blob then has to be re-packed by hand and nothing is trimmed.

The text of the strand lines is not carried: rows always write "+", so the round trip is byte-exact for files whose strand lines are "+".

This is the only module of the package that imports torch."""
import collections
import contextlib
import ctypes as C

import torch

from ._capi import SE, PE_TWO_FILES

U8, I32, MASK, OFFS = (torch.uint8,), (torch.int32,), (torch.bool, torch.uint8), (torch.int64, torch.uint64)


@contextlib.contextmanager
def _on_stream(codec, dev):
    """the context on torch's current stream of `dev` for the block, and back on its own stream afterwards, however the block ends"""
    codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        yield
    finally:
        codec.set_stream(None)


# the first eight fields are, in this order, the rows as every RfqCodec method takes them; a part that is absent, not looked at or empty is None
_Rows = collections.namedtuple("_Rows", "n L bases quals lens names names_len name_off dev U off_dtype")


def _rows_of(t, quals=False, names=False, pairs=False):
    """THE check of a rows dict, before any call: "bases" [n, L >= 1] uint8, contiguous, on a GPU; the other parts contiguous, of the dtype and the count that go
    with it, on the same device.  quals / names: True - required; None - taken when `t` has it ("name_off" decides for the names); False - not looked at.
    pairs: n must be even, and U = n / 2 units (else U = n).  -> _Rows."""
    bases = t["bases"]
    assert bases.dtype == torch.uint8 and bases.is_cuda and bases.dim() == 2 and bases.is_contiguous() and bases.shape[1] >= 1, "bases: [n, L] uint8, contiguous, on the GPU"
    n, L = int(bases.shape[0]), int(bases.shape[1])
    dev = bases.device
    assert not pairs or n % 2 == 0, "rows in pairs"
    p_q = p_n = p_o = off_dtype = None
    nl = 0
    if quals or (quals is None and t.get("quals") is not None):
        q = t["quals"]
        assert q.dtype == torch.uint8 and q.is_contiguous() and q.shape == bases.shape and q.device == dev, "quals: [n, L] uint8, contiguous, on the rows' device"
        p_q = q.data_ptr()
    if names or (names is None and t.get("name_off") is not None):
        blob, off = t["names"], t["name_off"]
        nl, off_dtype = blob.numel(), off.dtype
        p_n = _per(blob, None, dev, U8, "names: a uint8 blob (pack_names)")
        p_o = _per(off, n + 1, dev, OFFS, "name_off: [n + 1] int64")
    return _Rows(n, L, bases.data_ptr(), p_q, _per(t["lens"], n, dev, I32, "lens: [n] int32"), p_n, nl, p_o, dev, n // 2 if pairs else n, off_dtype)


def _per(x, count, dev, dtypes, what, optional=False):
    """THE check of a tensor with one entry per row or unit (or, count=None, of any size): dtype, contiguity, count and device -> its pointer; None for an
    optional tensor that is None and for an empty one (an empty tensor has no pointer to hand over)"""
    if x is None and optional:
        return None
    assert x is not None and x.dtype in dtypes and x.is_contiguous() and (count is None or x.numel() == count) and x.device == dev, what + ", contiguous, on the rows' device"
    return x.data_ptr() if x.numel() else None


def _triple(keep, start, length, n, dev):
    """select_rows' triple, checked, as the d_keep / d_start / d_len of a call (None: every row / 0 / to the end of the read)"""
    return dict(d_keep=_mask(keep, n, dev), d_start=_per(start, n, dev, I32, "start: [n] int32", True), d_len=_per(length, n, dev, I32, "length: [n] int32", True))


def _mask(keep, n, dev):
    return _per(keep, n, dev, MASK, "keep: [n] bool / uint8", True)


def _summary(r, fields):
    return {f: int(getattr(r, f)) for f in fields}


def _rows_out(prefix, m, L, nl, named, off_dtype, dev):
    """Five new tensors for m rows at stride L (and, named, nl name bytes with m + 1 offsets of off_dtype) -> the rows dict, the pointers and caps as the keyword
    arguments of the writing call (`prefix`: "d_" or "out_")"""
    out = {"bases": torch.empty((m, L), dtype=torch.uint8, device=dev), "quals": torch.empty((m, L), dtype=torch.uint8, device=dev),
           "lens": torch.empty((m,), dtype=torch.int32, device=dev)}
    kw = {prefix + "bases": out["bases"].data_ptr(), "bases_cap": m * L, prefix + "quals": out["quals"].data_ptr(), "quals_cap": m * L,
          prefix + "lens": out["lens"].data_ptr(), "lens_cap": m}
    if named:
        out["names"] = torch.empty((nl,), dtype=torch.uint8, device=dev); out["name_off"] = torch.zeros((m + 1,), dtype=off_dtype, device=dev)
        kw.update({prefix + "names": out["names"].data_ptr() if nl else None, "names_cap": nl, prefix + "name_off": out["name_off"].data_ptr(), "off_cap": m + 1})
    return out, kw


def decode_tensors(codec, rfq: torch.Tensor, row_len=None, codes=True, qual_offset=33, pad=255, names=False):
    """One .rfq image (a uint8 tensor on the codec's device) -> {"bases", "quals", "lens"}: row i = read i of the image in Repaq::decompress order
    (a PE file: rows 2k / 2k + 1 are R1 / R2 of pair k - `bases.view(-1, 2, L)`), padded with `pad` to L = row_len (None: the longest read).
    names=True adds "names" and "name_off" (decode_names).
    A size query and the decode, both ordered with torch's current stream; the context goes back to its own stream afterwards."""
    assert rfq.dtype == torch.uint8 and rfq.is_cuda and rfq.is_contiguous(), "rfq must be a contiguous uint8 tensor on the GPU"
    n = rfq.numel()
    with _on_stream(codec, rfq.device):
        q = codec.decode_rows(rfq.data_ptr(), n)
        L = max(int(q.max_len), 1) if row_len is None else int(row_len)
        rows = int(q.n_rows)
        out, kw = _rows_out("d_", rows, L, 0, False, None, rfq.device)
        if rows:
            codec.decode_rows(rfq.data_ptr(), n, row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad, pad_qual=pad, **kw)
    if names:
        out["names"], out["name_off"] = decode_names(codec, rfq)
    return out


def fastq_to_tensors(codec, fq1: torch.Tensor, fq2: torch.Tensor = None, paired=SE, row_len=None, codes=True, qual_offset=33, pad=255, names=True, final=True):
    """FASTQ text (uint8 tensors on the codec's device; fq2 with PE_TWO_FILES) -> {"bases", "quals", "lens", "names", "name_off", "consumed"}: row i = the
    i-th record the reference's reader makes of the text - the records encode() would take; two files: rows 2k / 2k + 1 are record k of fq1 / fq2 -,
    padded with `pad` to L = row_len (None: the longest read).  codes: A0 C1 G2 T3 N4 (any other base is refused; codes=False keeps the text's bytes,
    lower case and IUPAC included).  names=False leaves "names" / "name_off" out.  "consumed": (bytes of fq1, bytes of fq2) the rows cover - with
    final=False, or a text beyond one call's slice, the next call starts there.  A size query and one call, both ordered with torch's current stream;
    the context goes back to its own stream afterwards."""
    two = paired == PE_TWO_FILES
    for t in (fq1,) + ((fq2,) if two else ()):
        assert t is not None and t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous(), "fq1 / fq2 must be contiguous uint8 tensors on the GPU"
    dev = fq1.device
    src = dict(d_fq2=fq2.data_ptr() if two else None, n2=fq2.numel() if two else 0, paired=paired, final=final)
    with _on_stream(codec, dev):
        q = codec.text_rows(fq1.data_ptr(), fq1.numel(), **src)
        L = max(int(q.max_len), 1) if row_len is None else int(row_len)
        rows = int(q.n_rows)
        out, kw = _rows_out("d_", rows, L, int(q.names_len), names, torch.int64, dev)
        if rows:
            codec.text_rows(fq1.data_ptr(), fq1.numel(), row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad, pad_qual=pad, **kw, **src)
    out["consumed"] = (int(q.consumed1), int(q.consumed2))
    return out


def _compact(codec, t, call, kw_of, row_len, pad, more_of=None):
    """What select_rows, merge_pairs and group_rows share: `call` (RfqCodec.select_rows / merge_rows / group_rows) as a size query, then once more into five new
    tensors of exactly the reported sizes, both ordered with torch's current stream.  kw_of(n, dev) checks the caller's own inputs and returns the arguments they
    become; more_of(q, dev) makes the call's further outputs from the size query's result and returns the arguments of the writing call they become.  -> the last
    result struct, the rows dict ("bases", "quals", "lens" and, when `t` has them, "names" + "name_off")."""
    R = _rows_of(t, quals=True, names=None)
    kw = kw_of(R.n, R.dev)
    with _on_stream(codec, R.dev):
        q = call(*R[:8], **kw)
        L = max(int(q.max_len), 1) if row_len is None else int(row_len)
        m = int(q.n_rows)
        out, okw = _rows_out("out_", m, L, int(q.names_len), R.name_off is not None, R.off_dtype, R.dev)
        more = more_of(q, R.dev) if more_of is not None else {}
        if m:
            q = call(*R[:8], row_len=L, pad_base=pad, pad_qual=pad, **okw, **more, **kw)
    return q, out


def _tag_kw(tag, codes, n, dev):
    """select_rows' tag dict, checked, as the `tag` / `codes` of RfqCodec.select_rows"""
    from . import _capi as A
    unknown = set(tag) - {"start", "length", "sep", "prefix", "join", "at"}
    assert not unknown, "tag: unknown keys %s" % sorted(unknown)
    at = {"space": A.TAG_AT_SPACE, "end": A.TAG_AT_END}.get(tag.get("at", "space"))
    assert at is not None, 'tag: at is "space" or "end"'
    sep, join = str(tag.get("sep", ":")).encode(), str(tag.get("join", "_")).encode()
    assert len(sep) == 1 and len(join) == 1, "tag: sep and join are one byte each"
    assert n == 0 or (tag["start"].numel() == n and tag["length"].numel() == n), "tag: start and length are [n] int32"
    return dict(codes=codes, tag=dict(d_tag_start=_per(tag["start"], n, dev, I32, "tag start: [n] int32"), d_tag_len=_per(tag["length"], n, dev, I32, "tag length: [n] int32"),
                                      prefix=str(tag.get("prefix", "")).encode(), sep=sep, join=join, at=at))


def select_rows(codec, t, keep=None, start=None, length=None, pairs=False, min_len=1, row_len=None, pad=255, tag=None, codes=True):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "quals", "lens", optionally "names" + "name_off") -> a new dict with the same keys for the
    rows that are KEPT, each TRIMMED to bases [start, start + length) (rfq_select_rows), plus "dropped": {"mask", "short", "mate"}.  keep: [n] bool or uint8,
    non-zero = keep (None: every row); start / length: [n] int32 (None: 0 / to the end of the read); pairs: rows 2k / 2k + 1 stand or fall together; a row
    whose window is shorter than min_len is dropped (and with pairs its mate); rows are padded with `pad` to row_len (None: the longest kept window).  The
    bytes are the rows' own, names are kept whole - unless tag is given: {"start", "length": [n] int32 - the bases [start, start + length) of row i, at most 32,
    are its part of the tag, wherever they lie in the read -, optional "sep" (":"), "prefix" (""), "join" ("_"), "at" ("space" | "end")}: the kept names take
    sep, prefix + join, the part (with pairs both rows of a pair take R1's part, join, R2's part) in front of their first space, or at their end (rfq_name_tag);
    a unit whose parts are empty keeps its names.  codes: what the base rows were made with (looked at only with a tag).  A size query and one call, both ordered
    with torch's current stream; the context goes back to its own stream afterwards."""
    def kw_of(n, dev):
        return dict(pairs=pairs, min_len=min_len, **_triple(keep, start, length, n, dev), **(_tag_kw(tag, codes, n, dev) if tag is not None else {}))
    q, out = _compact(codec, t, codec.select_rows, kw_of, row_len, pad)
    out["dropped"] = {"mask": int(q.dropped_mask), "short": int(q.dropped_short), "mate": int(q.dropped_mate)}
    return out


def group_rows(codec, t, bin, n_bins, keep=None, start=None, length=None, pairs=False, rest=True, min_len=1, row_len=None, pad=255):
    """select_rows with the kept rows GROUPED by `bin` in ONE pass (rfq_group_rows): bin [U] int32, one entry per unit - a row, with pairs the rows 2k / 2k + 1;
    demux_rows' "sample" as it lies -, 0 .. n_bins - 1; a unit with bin < 0 goes to one more bin, the last (rest=True), or is dropped (rest=False); a bin >= n_bins
    is refused.  keep / start / length / pairs / min_len / row_len / pad: select_rows'.  -> select_rows' dict with the rows sorted by (bin, input row) - a stable
    sort, pairs stay adjacent -, plus "bin_off": [T + 1] int64 on the device, T = n_bins + rest, the first output row of every bin and the row count last, and
    "dropped": {"mask", "bin", "short", "mate"}.  The rows of bin b are rows [bin_off[b], bin_off[b + 1]) - what select_rows gives for the mask keep & (bin == b),
    byte for byte; group_parts cuts them out.  A size query and one call, both ordered with torch's current stream; the context goes back to its own stream
    afterwards."""
    T = int(n_bins) + (1 if rest else 0)
    box = {}

    def kw_of(n, dev):
        sel = _triple(keep, start, length, n, dev)
        assert not pairs or n % 2 == 0, "rows in pairs"
        return dict(pairs=pairs, min_len=min_len, d_bin=_per(bin, n // 2 if pairs else n, dev, I32, "bin: [U] int32"), n_bins=n_bins, rest=rest, **sel)

    def more_of(q, dev):
        box["bin_off"] = torch.zeros((T + 1,), dtype=torch.int64, device=dev)          # (no rows: every bin starts at 0, and nothing is called)
        return dict(out_bin_off=box["bin_off"].data_ptr(), bin_cap=T + 1)
    q, out = _compact(codec, t, codec.group_rows, kw_of, row_len, pad, more_of)
    out["bin_off"] = box["bin_off"]
    out["dropped"] = {"mask": int(q.dropped_mask), "bin": int(q.dropped_bin), "short": int(q.dropped_short), "mate": int(q.dropped_mate)}
    return out


def group_parts(g):
    """The bins of a group_rows result as a list of T entries, None for an empty bin, otherwise a dict of VIEWS of the result's tensors: "bases" / "quals" / "lens" -
    the bin's rows, which are contiguous -, and, where the rows have names, "names" - the bin's slice of the blob - and "name_off" - its offsets less the first (a
    slice of ONE new tensor that holds every bin's rows + 1 rebased offsets, made by a handful of torch calls whatever the number of bins).  rows_to_fastq and
    encode_tensors take an entry as it stands.  ONE read-back: bin_off, with the name offsets at those rows."""
    bin_off = g["bin_off"]
    named = g.get("name_off") is not None
    dev = bin_off.device
    noff = None
    if named:
        noff = g["name_off"] if g["name_off"].dtype == torch.int64 else g["name_off"].view(torch.int64)
    cut = (torch.stack([bin_off, noff[bin_off]]) if named else bin_off.unsqueeze(0)).cpu().tolist()
    rows = cut[0]
    used = [b for b in range(len(rows) - 1) if rows[b] != rows[b + 1]]
    at = {}                                                                   # bin -> where its rows + 1 offsets start in `flat`
    if named and used:
        counts = [rows[b + 1] - rows[b] + 1 for b in used]
        total = 0
        for b, c in zip(used, counts):
            at[b] = total; total += c
        meta = torch.tensor([counts, [rows[b] - at[b] for b in used], [cut[1][b] for b in used]], dtype=torch.int64).to(dev)
        src = torch.arange(total, device=dev) + torch.repeat_interleave(meta[1], meta[0], output_size=total)
        flat = noff[src] - torch.repeat_interleave(meta[2], meta[0], output_size=total)
    T = len(rows) - 1
    out = [None] * T
    if not used:
        return out

    def pieces(x, ends):                                                      # (one call cuts every view: a Python slice per bin and tensor costs more than the GPU's part of the call)
        return torch.tensor_split(x, ends) if ends else (x,)
    views = {k: pieces(g[k], rows[1:T]) for k in ("bases", "quals", "lens")}
    if named:
        views["names"] = pieces(g["names"], cut[1][1:T])
        offs = dict(zip(used, pieces(flat, [at[b] for b in used[1:]])))
    for b in used:
        out[b] = {k: v[b] for k, v in views.items()}
        if named:
            out[b]["name_off"] = offs[b]
    return out


SUMMARY_FIELDS = ("n_rows", "n_kept", "why_short", "why_n", "why_meanq", "why_lowq", "why_complex", "bases_in", "qsum_in", "q20_in", "q30_in", "bases_out", "qsum_out",
                  "q20_out", "q30_out")


def judge_rows(codec, t, codes=True, metrics=False, **criteria):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "quals", "lens"; codes: what they were made with) and the criteria of rfq_judge_rows
    (RfqCodec.judge_rows: trim_front, trim_tail, poly_g, cut_front / cut_right / cut_tail with cut_window and cut_mean_q, max_len, min_len, max_n, min_mean_q,
    qual_q + max_lowq_pct, min_complexity_pct) -> {"keep": [n] uint8, "start": [n] int32, "length": [n] int32, "why": [n] uint8 (the WHY_* bits of the reasons a
    row fails for), "summary": dict of the batch's counts} and, with metrics=True, "metrics": [n, 4] int32 (qsum, n_cnt, lowq, trans of the window).  keep, start
    and length are what select_rows takes.  "quals" must hold the scores (qual_offset taken off, as decode_tensors and fastq_to_tensors leave them).  One call,
    ordered with torch's current stream; the context goes back to its own stream afterwards."""
    R = _rows_of(t, quals=True)
    n, dev = R.n, R.dev
    keep = torch.empty((n,), dtype=torch.uint8, device=dev); why = torch.empty((n,), dtype=torch.uint8, device=dev)
    start = torch.empty((n,), dtype=torch.int32, device=dev); length = torch.empty((n,), dtype=torch.int32, device=dev)
    met = torch.empty((n, 4), dtype=torch.int32, device=dev) if metrics else None
    with _on_stream(codec, dev):
        r = codec.judge_rows(*R[:5], codes=codes, d_keep=keep.data_ptr(), d_start=start.data_ptr(), d_len=length.data_ptr(), d_why=why.data_ptr(),
                             d_metrics=met.data_ptr() if metrics else None, **criteria)
    out = {"keep": keep, "start": start, "length": length, "why": why, "summary": _summary(r, SUMMARY_FIELDS)}
    if metrics:
        out["metrics"] = met
    return out


ADAPTER_FIELDS = ("n_rows", "n_pairs", "pairs_found", "rows_cut", "rows_cut_overlap", "rows_cut_adapter", "bases_in", "bases_out")


def trim_adapters(codec, t, pairs=False, codes=True, adapter1=None, adapter2=None, min_overlap=30, max_diff=5, max_diff_pct=20, adapter_min=4, adapter_mm_per=8,
                  hist_len=0):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "lens"; codes: what they were made with) -> {"length": [n] int32 - what is left of each row
    after adapter removal (rfq_adapter_rows) -, "how": [n] uint8 (CUT_BY_OVERLAP | CUT_BY_ADAPTER), "summary": dict of the batch's counts}.  pairs: rows 2k /
    2k + 1 are R1 / R2; their overlap is searched (min_overlap, max_diff, max_diff_pct) and "insert" and "diff", [n / 2] int32 (insert -1: no overlap), are
    returned too.  adapter1 / adapter2: bytes of ACGT, at most 64 (None: off; with pairs adapter2 is the odd rows'), matched with adapter_min and adapter_mm_per
    (one mismatch per that many compared bases; 0: exact).  hist_len > 0 (pairs): "insert_hist", [hist_len] int64, the last bin holds every longer insert.
    "length" is select_rows' length (start 0) and, as "lens", what a later judge_rows takes.  One call, ordered with torch's current stream; the context goes
    back to its own stream afterwards."""
    R = _rows_of(t)
    assert not hist_len or pairs, "the insert-size histogram is for pairs"
    n, dev = R.n, R.dev
    length = torch.empty((n,), dtype=torch.int32, device=dev); how = torch.empty((n,), dtype=torch.uint8, device=dev)
    insert = torch.empty((n // 2,), dtype=torch.int32, device=dev) if pairs else None
    diff = torch.empty((n // 2,), dtype=torch.int32, device=dev) if pairs else None
    hist = torch.empty((hist_len,), dtype=torch.int64, device=dev) if hist_len else None
    crit = dict(min_overlap=min_overlap, max_diff=max_diff, max_diff_pct=max_diff_pct) if pairs else {}
    if adapter1 is not None or adapter2 is not None:
        crit.update(adapter_min=adapter_min, adapter_mm_per=adapter_mm_per)
    with _on_stream(codec, dev):
        r = codec.adapter_rows(n, R.L, R.bases, R.lens, codes=codes, pairs=pairs, adapter1=adapter1, adapter2=adapter2, hist_len=hist_len,
                               d_len=length.data_ptr(), d_how=how.data_ptr(), d_insert=insert.data_ptr() if pairs else None, d_diff=diff.data_ptr() if pairs else None,
                               d_insert_hist=hist.data_ptr() if hist_len else None, **crit)
    out = {"length": length, "how": how, "summary": _summary(r, ADAPTER_FIELDS)}
    if pairs:
        out["insert"], out["diff"] = insert, diff
    if hist_len:
        out["insert_hist"] = hist
    return out


MERGE_FIELDS = ("n_rows", "n_bases", "names_len", "max_len", "max_name", "n_pairs", "overlap_bases")


def merge_pairs(codec, t, insert, row_len=None, pad=255, unmerged=True, codes=True):
    """The paired rows of decode_tensors / fastq_to_tensors (`t`: "bases", "quals", "lens", optionally "names" + "name_off"; rows 2k / 2k + 1 are R1 / R2; codes:
    what they were made with) and trim_adapters' "insert" ([n / 2] int32, -1: no overlap) -> {"merged": a rows dict ("bases", "quals", "lens" and, when `t` has
    them, "names" + "name_off") with ONE row per pair whose insert is >= 0 - the fragment of insert bases: R1 from the front, the reverse complement of R2 from
    the back, the consensus of rfq_merge_rows where both cover a position, under R1's name -, "unmerged": select_rows of the other pairs, both mates (left out
    with unmerged=False), "summary": dict of the call's counts}.  `t` holds the lengths the insert was found on (not lengths cut further by an adapter match);
    narrow the choice with torch.where(cond, insert, -1).  Rows are padded with `pad` to row_len (None: the longest merged read).  "quals" must hold the scores.
    A size query and one call, both ordered with torch's current stream; the context goes back to its own stream afterwards."""
    def kw_of(n, dev):
        assert n % 2 == 0, "rows in pairs"
        return dict(d_insert=_per(insert, n // 2, dev, I32, "insert: [n / 2] int32"), codes=codes)
    q, merged = _compact(codec, t, codec.merge_rows, kw_of, row_len, pad)
    out = {"merged": merged, "summary": _summary(q, MERGE_FIELDS)}
    if unmerged:
        out["unmerged"] = select_rows(codec, t, keep=(insert < 0).repeat_interleave(2), pairs=True)
    return out


DEDUP_FIELDS = ("n_units", "n_candidates", "n_classes", "n_dups", "max_class", "bases_in", "bases_kept")


def dedup_rows(codec, t, pairs=False, key_len=0, best_qual=False, keep=None, hist_len=0):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "lens" and, with best_qual, "quals") -> {"keep": [n] uint8 - 1 for the rows of the ONE unit
    that is kept of every class of units with identical keys (rfq_dedup_rows), what select_rows takes -, "dup_of": [U] int32 (the unit index of the unit's
    representative, -1: no candidate), "count": [U] int32 (the class size at the representative, 0 elsewhere), "summary": dict of the batch's counts}.  A unit is
    a row (U = n), with pairs the rows 2k / 2k + 1 (U = n / 2); its key the first key_len bases (0: all) of each of its rows as they lie, the lengths included.
    The kept member is the lowest index, with best_qual the one with the highest score sum over its key (ties: the lowest index).  keep: [n] bool / uint8 - only
    units all of whose rows are non-zero there are looked at (judge_rows' "keep"); the others get keep 0, dup_of -1.  hist_len > 0: "hist", [hist_len] int64, bin
    c - 1 = classes of size c, the last bin every larger class.  One call, ordered with torch's current stream; the context goes back to its own stream afterwards."""
    R = _rows_of(t, quals=bool(best_qual), pairs=pairs)
    n, U, dev = R.n, R.U, R.dev
    d_in = _mask(keep, n, dev)
    out_keep = torch.empty((n,), dtype=torch.uint8, device=dev); dup_of = torch.empty((U,), dtype=torch.int32, device=dev)
    count = torch.empty((U,), dtype=torch.int32, device=dev)
    hist = torch.empty((hist_len,), dtype=torch.int64, device=dev) if hist_len else None
    with _on_stream(codec, dev):
        r = codec.dedup_rows(*R[:5], pairs=pairs, key_len=key_len, best_qual=best_qual, hist_len=hist_len, d_in=d_in, d_keep=out_keep.data_ptr(),
                             d_dup_of=dup_of.data_ptr(), d_count=count.data_ptr(), d_hist=hist.data_ptr() if hist_len else None)
    out = {"keep": out_keep, "dup_of": dup_of, "count": count, "summary": _summary(r, DEDUP_FIELDS)}
    if hist_len:
        out["hist"] = hist
    return out


PROFILE_TABLES = ("base_cnt", "base_qsum", "qual_hist", "len_hist", "meanq_hist", "gc_hist")
PROFILE_FIELDS = ("counted", "bases", "qsum", "q20", "q30", "gc", "other")


def profile_rows(codec, t, pairs=False, codes=True, keep=None, start=None, length=None, cycles=None, qbins=64, len_bins=None, tables=PROFILE_TABLES):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "quals", "lens"; codes: what they were made with) under select_rows' triple - keep: [n] bool /
    uint8 (None: every row), start / length: [n] int32 windows (None: 0 / to the end of the read), what judge_rows, trim_adapters and dedup_rows leave - -> the tables
    of a QC report (rfq_profile_rows), int64 each, M = 2 with pairs (row i is of mate i & 1: read 1 and read 2 apart), else 1: "base_cnt" / "base_qsum" [M, cycles, 5]
    (positions / score sum per cycle and class A C G T other), "qual_hist" [M, cycles, qbins], "len_hist" [M, len_bins], "meanq_hist" [M, qbins], "gc_hist" [M, 101];
    the last row / bin of each collects what lies beyond.  cycles / len_bins default to the rows' stride (+ 1 for the lengths); tables: the ones wanted.  "summary":
    n_rows, max_len (the longest counted window) and, per mate, lists of counted, bases, qsum, q20, q30, gc, other.  No row is moved.  One call, ordered with torch's
    current stream; the context goes back to its own stream afterwards."""
    R = _rows_of(t, quals=True, pairs=pairs)
    L, dev = R.L, R.dev
    sel = _triple(keep, start, length, R.n, dev)
    assert set(tables) <= set(PROFILE_TABLES), "tables: of " + ", ".join(PROFILE_TABLES)
    cycles = L if cycles is None else cycles; len_bins = L + 1 if len_bins is None else len_bins
    M = 2 if pairs else 1
    shapes = dict(base_cnt=(M, cycles, 5), base_qsum=(M, cycles, 5), qual_hist=(M, cycles, qbins), len_hist=(M, len_bins), meanq_hist=(M, qbins), gc_hist=(M, 101))
    out = {k: torch.empty(shapes[k], dtype=torch.int64, device=dev) for k in PROFILE_TABLES if k in tables}
    with _on_stream(codec, dev):
        r = codec.profile_rows(*R[:5], codes=codes, pairs=pairs, cycles=cycles, qbins=qbins, len_bins=len_bins, **sel, **{"d_" + k: v.data_ptr() for k, v in out.items()})
    out["summary"] = dict({f: [int(getattr(r, f)[m]) for m in range(M)] for f in PROFILE_FIELDS}, n_rows=int(r.n_rows), max_len=int(r.max_len))
    return out


SCREEN_BUILD_FIELDS = ("n_refs", "ref_bases", "n_positions", "n_kmers", "slots", "index_bytes")
SCREEN_FIELDS = ("n_units", "n_candidates", "n_matched", "n_kept", "kmers", "hits", "bases_in", "bases_kept")


def screen_index(codec, refs, k=25):
    """Reference sequences -> the index screen_rows takes (rfq_screen_build): the exact set of the canonical k-mers (k in 4 .. 31) of every reference; a k-mer lies
    inside ONE reference and is all ACGT, either case.  refs: a list of bytes / str (put on the codec's device), or a (blob, offsets) pair of device tensors - uint8
    and [n_refs + 1] int64, the layout of pack_names.  -> {"index": uint8 tensor (private bytes: which slot a k-mer lands in may differ from run to run, the set does
    not), "k", "n_kmers" (distinct values), "slots", "summary": dict of the call's counts}.  One index per reference set; for per-reference counts build one index
    per reference.  A size query and one call, both ordered with torch's current stream; the context goes back to its own stream afterwards."""
    if isinstance(refs, tuple):
        blob, off = refs
    else:
        blob, off = pack_names([r.encode() if isinstance(r, str) else bytes(r) for r in refs], torch.device("cuda", codec.device))
    assert blob.dtype == torch.uint8 and blob.is_cuda and blob.is_contiguous(), "refs: a contiguous uint8 blob on the GPU"
    assert off.dtype in (torch.int64, torch.uint64) and off.is_contiguous() and off.numel() >= 1 and off.device == blob.device, "offsets: [n_refs + 1] int64 on the blob's device"
    n_refs = off.numel() - 1
    # (references of no bytes at all are still references: the call wants a pointer for them, and an empty tensor has none)
    at = blob if blob.numel() else torch.zeros((1,), dtype=torch.uint8, device=blob.device)
    src = (at.data_ptr(), blob.numel(), off.data_ptr(), n_refs)
    with _on_stream(codec, blob.device):
        q = codec.screen_build(*src, k=k, size_only=True)
        index = torch.empty((int(q.index_bytes),), dtype=torch.uint8, device=blob.device)
        r = codec.screen_build(*src, k=k, d_index=index.data_ptr(), index_cap=index.numel())
    return {"index": index, "k": k, "n_kmers": int(r.n_kmers), "slots": int(r.slots), "summary": _summary(r, SCREEN_BUILD_FIELDS)}


def screen_rows(codec, t, index, pairs=False, codes=True, keep=None, min_hits=1, min_pct=0, keep_matched=False):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "lens"; codes: what they were made with) against screen_index's index (the dict, or its "index"
    tensor) -> {"keep": [n] uint8 - what dedup_rows takes as keep and select_rows as keep -, "hits": [n] int32 (the row's k-mers whose canonical value is in the
    set), "kmers": [n] int32 (its valid k-mers), "summary": dict of the batch's counts} (rfq_screen_rows).  A unit is a row, with pairs the rows 2k / 2k + 1; with H
    and K its hits and k-mers over its rows it matches when H >= max(min_hits, 1) and 100 * H >= min_pct * K.  A unit that matches is dropped - a contaminant -,
    with keep_matched it is the one that stays - a bait.  keep: [n] bool / uint8 - only units all of whose rows are non-zero there are looked at (judge_rows'
    "keep"); the others get 0 / 0 / 0.  "lens" may be what trim_adapters or judge_rows left.  One call, ordered with torch's current stream; the context goes back
    to its own stream afterwards."""
    index = index["index"] if isinstance(index, dict) else index
    R = _rows_of(t, pairs=pairs)
    n, dev = R.n, R.dev
    p_ix = _per(index, None, dev, U8, "index: screen_index's uint8 tensor")
    d_in = _mask(keep, n, dev)
    out_keep = torch.empty((n,), dtype=torch.uint8, device=dev)
    hits = torch.empty((n,), dtype=torch.int32, device=dev); kmers = torch.empty((n,), dtype=torch.int32, device=dev)
    with _on_stream(codec, dev):
        r = codec.screen_rows(n, R.L, R.bases, R.lens, p_ix, index.numel(), codes=codes, pairs=pairs, min_hits=min_hits, min_pct=min_pct, keep_matched=keep_matched,
                              d_in=d_in, d_kmers=kmers.data_ptr(), d_hits=hits.data_ptr(), d_keep=out_keep.data_ptr())
    return {"keep": out_keep, "hits": hits, "kmers": kmers, "summary": _summary(r, SCREEN_FIELDS)}


KMERS_ROWS_FIELDS = ("n_rows", "n_counted", "bases_in", "added", "n_new", "n_kmers", "total", "lost")
KMERS_READ_FIELDS = ("k", "slots", "n_kmers", "total", "max_count", "n_selected", "selected_total", "index_slots", "index_bytes")


def kmer_table(codec, k=25, slots=1 << 20):
    """An empty table of canonical k-mers (k in 4 .. 31) with counts, which count_kmers adds to and kmer_counts reads (rfq_kmers_init) -> {"table": uint8 tensor on
    the codec's device (private bytes: which slot a k-mer lands in may differ from run to run, the counts do not), "k", "slots"}.  slots: at least twice the
    distinct values expected - the power of two >= max(1024, slots) is taken, 16 bytes a slot; a table that turns out too small refuses the count and has to be
    made again.  The table outlives the calls: count the batches of a file into one.  A size query and one call, both ordered with torch's current stream; the
    context goes back to its own stream afterwards."""
    dev = torch.device("cuda", codec.device)
    with _on_stream(codec, dev):
        q = codec.kmers_init(k=k, slots=slots, size_only=True)
        table = torch.empty((int(q.table_bytes),), dtype=torch.uint8, device=dev)
        r = codec.kmers_init(k=k, slots=slots, d_table=table.data_ptr(), table_cap=table.numel())
    return {"table": table, "k": k, "slots": int(r.slots)}


def count_kmers(codec, t, table, codes=True, keep=None):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "lens"; codes: what they were made with) into kmer_table's table (the dict, or its "table"
    tensor): 1 is added to the count of the canonical value of every valid k-mer of every counted row (rfq_kmers_rows) -> {"kmers": [n] int32 (the row's valid
    k-mers, what screen_rows' "kmers" holds; 0 for a row that is not counted), "summary": dict of the call's counts - added, n_new, and the table's n_kmers and
    total after the call}.  keep: [n] bool / uint8 - only rows that are non-zero there are counted (judge_rows' "keep"; rows, not pairs).  "lens" may be what
    trim_adapters or judge_rows left.  Calls on one table add up, in any order; ONE call at a time on a table.  One call, ordered with torch's current stream; the
    context goes back to its own stream afterwards."""
    table = table["table"] if isinstance(table, dict) else table
    R = _rows_of(t)
    n, dev = R.n, R.dev
    p_tab = _per(table, None, dev, U8, "table: kmer_table's uint8 tensor")
    d_in = _mask(keep, n, dev)
    kmers = torch.empty((n,), dtype=torch.int32, device=dev)
    with _on_stream(codec, dev):
        r = codec.kmers_rows(n, R.L, R.bases, R.lens, p_tab, table.numel(), codes=codes, d_in=d_in, d_kmers=kmers.data_ptr())
    return {"kmers": kmers, "summary": _summary(r, KMERS_ROWS_FIELDS)}


def kmer_counts(codec, table, min_count=1, max_count=0, hist_len=0, index=False):
    """What kmer_table's table holds (rfq_kmers_read) -> {"values": [m] int64, "counts": [m] int64 - the entries with max(min_count, 1) <= count and (max_count ==
    0 or count <= max_count), SORTED by value (torch.sort: the C call leaves their order open), a value the 2k bits of the canonical k-mer, the first base highest -,
    "hist": [hist_len] int64 or None - bin c - 1 = the distinct values seen c times over ALL entries, the last bin every larger count: the k-mer spectrum -, "index":
    with index=True the dict screen_rows takes - a screen index of the selected values, the bridge to screening by abundance -, else None, "summary": dict of the
    read's counts}.  The most frequent k-mers are torch.topk on "counts".  A size query and one call, both ordered with torch's current stream; the context goes
    back to its own stream afterwards."""
    table = table["table"] if isinstance(table, dict) else table
    assert table.dtype == torch.uint8 and table.is_cuda and table.is_contiguous(), "table: kmer_table's uint8 tensor on the GPU"
    dev = table.device
    tb = (table.data_ptr(), table.numel())
    with _on_stream(codec, dev):
        q = codec.kmers_read(*tb, min_count=min_count, max_count=max_count, size_only=True)
        m = int(q.n_selected)
        values = torch.empty((m,), dtype=torch.int64, device=dev); counts = torch.empty((m,), dtype=torch.int64, device=dev)
        hist = torch.empty((hist_len,), dtype=torch.int64, device=dev) if hist_len else None
        ix = torch.empty((int(q.index_bytes),), dtype=torch.uint8, device=dev) if index else None
        # (an empty tensor has no pointer to hand over: no list is asked for then)
        r = codec.kmers_read(*tb, min_count=min_count, max_count=max_count, hist_len=hist_len, d_hist=hist.data_ptr() if hist_len else None,
                             d_values=values.data_ptr() if m else None, d_counts=counts.data_ptr() if m else None, list_cap=m,
                             d_index=ix.data_ptr() if index else None, index_cap=ix.numel() if index else 0)
    values, order = torch.sort(values)
    counts = counts[order]
    out_index = {"index": ix, "k": int(r.k), "n_kmers": m, "slots": int(r.index_slots)} if index else None
    return {"values": values, "counts": counts, "hist": hist, "index": out_index, "summary": _summary(r, KMERS_READ_FIELDS)}


DEMUX_FIELDS = ("n_units", "n_candidates", "n_assigned", "n_samples", "n_exact", "why_none", "why_ambig", "why_short", "why_combo", "bases_in", "bases_out")


def demux_rows(codec, t, barcodes1, barcodes2=None, sheet=None, pairs=False, codes=True, keep=None, off1=0, off2=0, skip1=0, skip2=0, max_mm=1, min_delta=1):
    """The rows of decode_tensors / fastq_to_tensors (`t`: "bases", "lens"; codes: what they were made with) against one or two sets of inline barcodes
    (rfq_demux_rows) -> {"sample": [U] int32 (the unit's sample, -1: none), "why": [U] uint8 (the DEMUX_* bits of repaq_amd._capi: 1 no barcode within max_mm,
    2 ambiguous, 4 the read ends in front of the window's end, 8 both matched but the pair is not in the sheet, 128 masked by `keep`), "best": [n] int32 (the row's
    nearest barcode, -1 where nothing was compared), "dist": [n] uint8 (its distance, 255 where best is -1), "keep": [n] uint8 and "start": [n] int32 - what
    select_rows and split_rows take: 1 and the first base behind barcode and linker for the rows of an assigned unit, 0 and 0 otherwise -, "counts": [n_samples + 1]
    int64 (the candidate units per sample, last the unassigned), "summary": dict of the batch's counts}.  A unit is a row, with pairs the rows 2k / 2k + 1 (U units);
    "sample" is what group_rows takes as bin and split_rows as sample.
    barcodes1 / barcodes2: a list of str / bytes of ONE length per set (1 .. 32 bases, at most 4096, A C G T), read at [off, off + len) of R1 / R2; barcodes2 and
    sheet need pairs.  sheet: a list of (i, j), sample s the pair listed s-th; None: every combination, sample i * n2 + j.  A row matches with d1 <= max_mm and
    d2 - d1 >= min_delta, d1 / d2 the Hamming distances of the best and the second-best barcode (an N never agrees; min_delta=0 lets the lowest index win a tie).
    skip1 / skip2: linker bases cut with the barcode.  keep: [n] bool / uint8 - only units all of whose rows are non-zero there are looked at.  Barcodes of
    several lengths in one set, indels, barcodes at other places than a fixed offset from the read's start, N as a wildcard, barcodes in the name line and UMIs are
    not offered.  One call, ordered with torch's current stream; the context goes back to its own stream afterwards."""
    R = _rows_of(t, pairs=pairs)
    n, U, dev = R.n, R.U, R.dev
    d_in = _mask(keep, n, dev)
    n_samples = len(barcodes1) if barcodes2 is None else (len(sheet) if sheet is not None else len(barcodes1) * len(barcodes2))
    sample = torch.empty((U,), dtype=torch.int32, device=dev); why = torch.empty((U,), dtype=torch.uint8, device=dev)
    best = torch.empty((n,), dtype=torch.int32, device=dev); dist = torch.empty((n,), dtype=torch.uint8, device=dev)
    out_keep = torch.empty((n,), dtype=torch.uint8, device=dev); start = torch.empty((n,), dtype=torch.int32, device=dev)
    counts = torch.empty((n_samples + 1,), dtype=torch.int64, device=dev)
    with _on_stream(codec, dev):
        r = codec.demux_rows(n, R.L, R.bases, R.lens, barcodes1, barcodes2, sheet, codes=codes, pairs=pairs, off1=off1, off2=off2, skip1=skip1, skip2=skip2,
                             max_mm=max_mm, min_delta=min_delta, d_in=d_in, d_sample=sample.data_ptr(), d_why=why.data_ptr(),
                             d_best=best.data_ptr(), d_dist=dist.data_ptr(), d_keep=out_keep.data_ptr(), d_start=start.data_ptr(), d_counts=counts.data_ptr())
    return {"sample": sample, "why": why, "best": best, "dist": dist, "keep": out_keep, "start": start, "counts": counts, "summary": _summary(r, DEMUX_FIELDS)}


def split_rows(codec, t, sample, n_samples, start=None, length=None, pairs=False, unassigned=True, **select_kw):
    """The rows of `t` by sample: one select_rows call per sample, the keep mask `sample == s` made on the device (with pairs spread to both rows of a pair by a torch
    index) -> a list of n_samples select_rows results, entry s the rows of sample s, and with unassigned=True one more, last, for the units with sample < 0.  Only
    the bins that hold a unit get a call (one torch.bincount and one read-back say which); the others are None.  sample: demux_rows' "sample" ([U] int32); start /
    length: what select_rows takes - demux_rows' "start" cuts barcode and linker off the assigned rows and leaves the unassigned ones whole -; select_kw: min_len,
    row_len, pad.  select_rows' min_len = 1 holds here too: a unit one of whose rows has nothing left behind its start (barcode, prefix and linker took the whole read,
    or an unassigned mate is empty) is dropped from its bin with both rows, so a bin may hold fewer units than demux_rows' "counts" says - the result's "dropped" counts them;
    min_len=0 keeps them, as rows of length 0 that rows_to_fastq and encode_tensors refuse.  A select_rows pass reads a mask byte and a few words per row and moves only the rows it keeps, so a pass per sample is cheap beside moving the rows
    once (DESIGN.md has the measured time).  group_rows + group_parts give the same bins in ONE pass over the rows."""
    R = _rows_of(t, pairs=pairs)
    n, dev = R.n, R.dev
    _per(sample, R.U, dev, I32, "sample: [U] int32")
    bins = torch.where(sample >= 0, sample, torch.full_like(sample, n_samples)).to(torch.int64)
    have = torch.bincount(bins, minlength=n_samples + 1).cpu().tolist()
    unit_of = torch.arange(n, device=dev) // 2 if pairs else None
    out = []
    for s in range(n_samples + (1 if unassigned else 0)):
        if not have[s]:
            out.append(None)
            continue
        mask = bins == s
        mask = (mask[unit_of] if pairs else mask).to(torch.uint8).contiguous()
        out.append(select_rows(codec, t, keep=mask, start=start, length=length, pairs=pairs, **select_kw))
    return out


def filter_rows(codec, t, pairs=False, codes=True, min_len=1, row_len=None, pad=255, **criteria):
    """judge_rows with the criteria, then select_rows with its keep mask and windows and the same min_len: the dict of select_rows (the kept rows, trimmed and
    compacted, with their names) plus "summary" (the judge's: every row on its own, before the pair rule)."""
    j = judge_rows(codec, t, codes=codes, min_len=min_len, **criteria)
    out = select_rows(codec, t, keep=j["keep"], start=j["start"], length=j["length"], pairs=pairs, min_len=min_len, row_len=row_len, pad=pad)
    out["summary"] = j["summary"]
    return out


def decode_names(codec, rfq: torch.Tensor):
    """One .rfq image -> (blob, offsets): the name lines of its reads back to back ('@' included, no line breaks) as a uint8 tensor and their n + 1 int64
    offsets - the names / name_off of encode_tensors and rows_to_fastq, row i = row i of decode_tensors (rfq_decode_names: the chunk table, the name
    sections and the coordinate streams are read, none of the bases or qualities).  The text of the strand lines is not carried.  One call with
    context-owned results, copied into tensors of the caller's; ordered with torch's current stream."""
    assert rfq.dtype == torch.uint8 and rfq.is_cuda and rfq.is_contiguous(), "rfq must be a contiguous uint8 tensor on the GPU"
    with _on_stream(codec, rfq.device):
        r = codec.decode_names(rfq.data_ptr(), rfq.numel())
        blob = _own_copy(codec, r.d_names, int(r.names_len), rfq.device)
        off = _own_copy(codec, r.d_name_off, 8 * (int(r.n_rows) + 1), rfq.device).view(torch.int64)
    return blob, off


def pack_names(names, device):
    """a list of name lines (bytes, '@' included, no line breaks) -> (blob, offsets): the lines back to back as a uint8 tensor and their n + 1 int64
    offsets, both on `device` - the names / name_off of encode_tensors and rows_to_fastq"""
    import numpy as np
    n = len(names)
    off = np.zeros(n + 1, dtype=np.int64)
    if n:
        off[1:] = np.cumsum(np.fromiter((len(x) for x in names), dtype=np.int64, count=n))
    blob = np.frombuffer(b"".join(names), dtype=np.uint8)
    return torch.from_numpy(blob.copy()).to(device), torch.from_numpy(off).to(device)


def _own_copy(codec, d_ptr, n, device):
    """a tensor of the caller's with the n bytes at d_ptr (a result buffer of the context), copied on torch's current stream"""
    out = torch.empty((n,), dtype=torch.uint8, device=device)
    if n:
        codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(out.data_ptr()), C.c_void_p(d_ptr), n))
    return out


def encode_tensors(codec, bases, quals, lens, names, name_off, paired=SE, chunk_bases=1_000_000, codes=True, qual_offset=33, final=True,
                   emit_header=True, flush_all=False):
    """Rows in the layout of decode_tensors (+ the names: pack_names) -> the .rfq image as a uint8 tensor, by rfq_encode_rows: the text is made
    and encoded on the GPU.  A PE file: rows 2k / 2k + 1 are R1 / R2 of pair k.  Several batches make one file: the first with flush_all=True,
    final=False, the last with emit_header=False.  Ordered with torch's current stream; the context goes back to its own stream afterwards."""
    R = _rows_of(dict(bases=bases, quals=quals, lens=lens, names=names, name_off=name_off), quals=True, names=True)
    with _on_stream(codec, R.dev):
        r = codec.encode_rows(*R[:8], paired=paired, codes=codes, qual_offset=qual_offset, chunk_bases=chunk_bases, final=final, emit_header=emit_header,
                              flush_all=flush_all)
        return _own_copy(codec, r.d_rfq, int(r.rfq_len), R.dev)


def rows_to_fastq(codec, bases, quals, lens, names, name_off, paired=SE, codes=True, qual_offset=33):
    """The same rows -> the FASTQ text as a uint8 tensor (rfq_rows_to_text, written straight into the tensor); a pair of tensors with PE_TWO_FILES
    (rows 2k -> the first, rows 2k + 1 -> the second).  Ordered with torch's current stream."""
    R = _rows_of(dict(bases=bases, quals=quals, lens=lens, names=names, name_off=name_off), quals=True, names=True)
    with _on_stream(codec, R.dev):
        q = codec.rows_to_text(*R[:8], paired=paired, codes=codes, qual_offset=qual_offset, size_only=True)
        n1, n2 = int(q.n1), int(q.n2)
        # (16 bytes more than the text: torch's allocations are 16-byte aligned, and the slack keeps a later rfq_encode_batch on the tensor inside it)
        t1 = torch.empty((n1 + 16,), dtype=torch.uint8, device=R.dev)
        t2 = torch.empty((n2 + 16,), dtype=torch.uint8, device=R.dev) if paired == PE_TWO_FILES else None
        if R.n:
            codec.rows_to_text(*R[:8], paired=paired, codes=codes, qual_offset=qual_offset, d_out1=t1.data_ptr(), cap1=n1 + 16,
                               d_out2=t2.data_ptr() if t2 is not None else None, cap2=n2 + 16 if t2 is not None else 0)
    return (t1[:n1], t2[:n2]) if paired == PE_TWO_FILES else t1[:n1]


# extract_umi lives in repaq_amd/umi.py (it makes no call of its own: two arrays with torch ops, then select_rows) and is offered here beside select_rows
from .umi import extract_umi  # noqa: E402,F401
