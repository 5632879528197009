"""UMI extraction on the rows of repaq_amd.tensors: extract_umi builds the two arrays of select_rows' tag with torch ops on the device and calls select_rows (rfq_select_rows
with an rfq_name_tag).  Offered as repaq_amd.tensors.extract_umi; torch is imported when the function is called."""


def extract_umi(codec, t, loc, umi_len, umi_skip=0, prefix="", sep=":", start=None, keep=None, pairs=False, codes=True, min_len=1, row_len=None, pad=255):
    """UMI extraction in the manner of fastp's --umi / umi_tools extract: the UMI leaves the read and goes into its name.  loc: "read1" - the UMI is at the front of
    every row (with pairs: of R1, rows 2k), "read2" - of R2, "per_read" - of both mates (the name takes R1's, "_", R2's); the last two need pairs.  umi_len bases
    from `start` ([n] int32 - demux_rows' "start": a UMI behind a barcode -, None: 0) are the UMI, umi_skip more are cut off behind them; prefix / sep: fastp's
    --umi_prefix and the byte in front of the tag (names end ":UMI_ACGT" - here "<sep><prefix>_<umi>", in front of the name's first space).  A read too short
    gives a shorter tag, never a refusal: tl = clamp(min(umi_len, lens - start), 0), the new window starts at min(lens, start + tl + umi_skip); a row `loc` does
    not name gives no part and keeps its bases from `start` on.  keep / pairs /
    min_len / row_len / pad: select_rows'; codes: what the base rows were made with.  The two arrays are made with torch ops on the device, no host sync.
    -> select_rows' dict.  An inline UMI is already part of dedup_rows' key when dedup runs BEFORE this step (the bases are still in the read); UMI-aware
    near-duplicate removal, UMIs read out of the name line and UMI quality filters are not built; umi_len is at most 32."""
    import torch
    from .tensors import select_rows, _rows_of, _per, I32
    _rows_of(t, quals=True, names=None, pairs=pairs)                          # (the rows dict is checked before any torch op looks at it)
    assert loc in ("read1", "read2", "per_read"), 'loc is "read1", "read2" or "per_read"'
    assert pairs or loc == "read1", 'loc "%s" needs pairs' % loc
    assert 0 < int(umi_len) <= 32 and int(umi_skip) >= 0, "umi_len is 1 .. 32, umi_skip >= 0"
    lens = t["lens"]
    _per(start, lens.numel(), lens.device, I32, "start: [n] int32", True)
    ts = torch.zeros_like(lens) if start is None else torch.minimum(start, lens)      # (a start behind the read: an empty part at the read's end)
    tl = torch.clamp(torch.clamp(lens - ts, max=int(umi_len)), min=0)
    skip = torch.full_like(lens, int(umi_skip))
    if pairs and loc != "per_read":                                          # the rows `loc` does not name give no part and lose nothing
        named = (torch.arange(lens.numel(), device=lens.device, dtype=torch.int32) & 1) == (0 if loc == "read1" else 1)
        tl = torch.where(named, tl, torch.zeros_like(tl)); skip = torch.where(named, skip, torch.zeros_like(skip))
    new_start = torch.minimum(lens, ts + tl + skip).to(torch.int32)
    return select_rows(codec, t, keep=keep, start=new_start, pairs=pairs, min_len=min_len, row_len=row_len, pad=pad, codes=codes,
                       tag=dict(start=ts.to(torch.int32).contiguous(), length=tl.to(torch.int32).contiguous(), prefix=prefix, sep=sep))
