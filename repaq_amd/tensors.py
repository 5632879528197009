"""Decoded reads as torch tensors on the GPU (rfq_decode_rows): what a model, a k-mer counter or a quality filter takes.

    from repaq_amd import RfqCodec
    from repaq_amd.tensors import decode_tensors
    codec = RfqCodec(device=0)
    rfq = torch.from_file("x.rfq", size=n, dtype=torch.uint8).cuda()
    t = decode_tensors(codec, rfq)            # {"bases": [n, L] uint8 codes A0 C1 G2 T3 N4, "quals": [n, L] Phred, "lens": [n] int32}

This is the only module of the package that imports torch."""
import torch


def decode_tensors(codec, rfq: torch.Tensor, row_len=None, codes=True, qual_offset=33, pad=255):
    """One .rfq image (a uint8 tensor on the codec's device) -> {"bases", "quals", "lens"}: row i = read i of the image in Repaq::decompress order
    (a PE file: rows 2k / 2k + 1 are R1 / R2 of pair k - `bases.view(-1, 2, L)`), padded with `pad` to L = row_len (None: the longest read).
    A size query and the decode, both ordered with torch's current stream; the context goes back to its own stream afterwards."""
    assert rfq.dtype == torch.uint8 and rfq.is_cuda and rfq.is_contiguous(), "rfq must be a contiguous uint8 tensor on the GPU"
    n = rfq.numel()
    codec.set_stream(torch.cuda.current_stream(rfq.device).cuda_stream)
    try:
        q = codec.decode_rows(rfq.data_ptr(), n)
        L = max(int(q.max_len), 1) if row_len is None else int(row_len)
        rows = int(q.n_rows)
        bases = torch.empty((rows, L), dtype=torch.uint8, device=rfq.device)
        quals = torch.empty((rows, L), dtype=torch.uint8, device=rfq.device)
        lens = torch.empty((rows,), dtype=torch.int32, device=rfq.device)
        if rows:
            codec.decode_rows(rfq.data_ptr(), n, row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad, pad_qual=pad,
                              d_bases=bases.data_ptr(), bases_cap=rows * L, d_quals=quals.data_ptr(), quals_cap=rows * L,
                              d_lens=lens.data_ptr(), lens_cap=rows)
    finally:
        codec.set_stream(None)
    return {"bases": bases, "quals": quals, "lens": lens}
