// dec/rows.h - reads as fixed-stride rows (rfq_decode_rows): every read's bases and qualities from the expanded stage's qdec / sdec
// Part of rfq_decode_kernels.h (included from there, last; not a stand-alone header).
#pragma once
// The per-read logic is emit_one's (dec/emit_expanded.h): overlap re-expansion from sb[sp - ov + p] (a positive overlap: the borrowed part
// sits right in front of the read's own stored bases) or from the mate's stored bases (negative: sb[sp - prevlen + p - keep]), reverse
// complement of the odd reads of an interleaved chunk, implied N where the quality equals the header's N quality.  Row i = read i of the call.
struct RowsOut {
    uint8_t* bases; uint8_t* quals; int32_t* lens;    // [n_rows][row_len], [n_rows][row_len], [n_rows]; any of them null = not wanted
    uint64_t row_len, n_rows;
    uint32_t codes;                                   // bases as A0 C1 G2 T3 N4 instead of their ASCII bytes
    uint32_t qoff4, pad_b4, pad_q4;                   // quality offset / pad bytes, repeated in the four bytes of a word
    uint32_t vec;                                     // row_len % 16 == 0 and both row buffers 16-byte aligned: one 16-byte store per group
};
// A C G T N -> 0 1 2 3 4: bits 1-3 of the ASCII byte (A 0, C 1, T 2, G 3, N 7) index an 8-entry table, four bytes in one v_perm_b32
__device__ __forceinline__ uint32_t code4_acgtn(uint32_t w) { return __builtin_amdgcn_perm(0x04000000u, 0x02030100u, (w >> 1) & 0x07070707u); }
// 16 bytes at any alignment: five aligned words and a funnel shift (reads up to 3 bytes in front of p and 4 behind p + 16: both inside the
// 256-byte-aligned qdec / sdec allocations, whose last chunk is followed by >= 256 bytes of slack)
__device__ __forceinline__ void ld16_any(const uint8_t* p, uint32_t (&w)[4]) {
    const uint32_t* a = (const uint32_t*)((uintptr_t)p & ~(uintptr_t)3); const uint32_t sh = 8u * (uint32_t)((uintptr_t)p & 3u);
    uint32_t v[5];
#pragma unroll
    for (int i = 0; i < 5; i++) v[i] = a[i];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)((((uint64_t)v[i + 1] << 32) | v[i]) >> sh);
}
// grid (bx, n_chunks), 256 threads.  A workgroup owns a run of a chunk's reads; a thread owns one 16-byte group [k0, k0 + 16) of one row at a
// time, in GroupWalk's order (rfq_common.h), and stores it once (store_group16).
__global__ void __launch_bounds__(256) k_dec_rows(const DChunk* __restrict__ CH, const DevHeader* __restrict__ D, DReadTab R,
                                                  const uint64_t* __restrict__ qbase, const uint64_t* __restrict__ sbase,
                                                  const uint8_t* __restrict__ qdec, const uint8_t* __restrict__ sdec, RowsOut o) {
    const uint32_t c = blockIdx.y; const DChunk d = CH[c];
    const bool il = (d.flags & C_PE_INTERLEAVED) != 0, implied_n = !(D->flags & H_N_POS);
    const uint32_t nq = D->n_base_qual & 0xFFu, nq4 = nq * 0x01010101u;
    const uint32_t f = d.rbase, pq0 = R.pq[f], pv0 = R.pv[f].d;
    const uint8_t* const qc = qdec + qbase[c]; const uint8_t* const sc = sdec + sbase[c];
    const uint32_t per = (d.reads + gridDim.x - 1) / gridDim.x;
    const uint32_t rs = blockIdx.x * per < d.reads ? blockIdx.x * per : d.reads, nr = (rs + per < d.reads ? rs + per : d.reads) - rs;
    for (GroupWalk w(o.row_len, blockDim.x); w.j < nr; w.step()) {
        const uint32_t k = w.k, r = rs + w.j, g = f + r; const uint64_t row = (uint64_t)d.rbase_abs + r;
        if (row >= o.n_rows) break;                                          // (the walk's read count bounds the rows: never past the caller's buffers)
        const uint32_t len = R.len[g]; const int ov = R.ov[g]; const bool rc = il && (r & 1u);
        const uint32_t k0 = 16u * k;
        if (k == 0 && o.lens) o.lens[row] = (int32_t)len;
        const uint8_t* const qs = qc + (R.pq[g] - pq0);                      // the read's qualities, interleaved orientation
        const uint8_t* const ss = sc + (R.pv[g].d - pv0);                    // its first stored base
        // a negative overlap borrows positions [keep, len) from the end of the mate's stored bases; a positive one keeps them contiguous
        const uint32_t keep = ov < 0 ? len - (uint32_t)(-ov) : len, prevlen = ov < 0 ? R.len[g - 1] : 0u;
        const uint8_t* const sa = ss - (ov > 0 ? ov : 0); const uint8_t* const sb = ss - prevlen - keep;    // base at p: sa[p] (p < keep), sb[p] (p >= keep)
        uint32_t wb[4] = { o.pad_b4, o.pad_b4, o.pad_b4, o.pad_b4 }, wq[4] = { o.pad_q4, o.pad_q4, o.pad_q4, o.pad_q4 };
        if (k0 < len) {
            // a whole group from one source run, word-wise: interleaved-orientation positions [p0, p0 + 16), back to front for an RC mate
            const uint8_t* sp = nullptr; uint32_t p0 = 0;
            if (k0 + 16u <= len) {
                p0 = rc ? len - 16u - k0 : k0;
                if (p0 + 16u <= keep) sp = sa + p0;
                else if (p0 >= keep) sp = sb + p0;
            }
            if (sp) {
                ld16_any(qs + p0, wq);
                if (o.bases) {
                    ld16_any(sp, wb);
                    if (implied_n) {
#pragma unroll
                        for (int i = 0; i < 4; i++) { const uint32_t mk = eq_bytes_full(wq[i], nq4); wb[i] = (wb[i] & ~mk) | (0x4E4E4E4Eu & mk); }
                    }
                    if (rc) { const uint32_t x0 = bswap32(wb[3]), x1 = bswap32(wb[2]), x2 = bswap32(wb[1]), x3 = bswap32(wb[0]);
                              wb[0] = comp4_acgtn(x0); wb[1] = comp4_acgtn(x1); wb[2] = comp4_acgtn(x2); wb[3] = comp4_acgtn(x3); }
                    if (o.codes) {
#pragma unroll
                        for (int i = 0; i < 4; i++) wb[i] = code4_acgtn(wb[i]);
                    }
                }
                if (rc) { const uint32_t x0 = bswap32(wq[3]), x1 = bswap32(wq[2]), x2 = bswap32(wq[1]), x3 = bswap32(wq[0]); wq[0] = x0; wq[1] = x1; wq[2] = x2; wq[3] = x3; }
#pragma unroll
                for (int i = 0; i < 4; i++) wq[i] = sub_bytes(wq[i], o.qoff4);
            } else {
                // the read's last, partial group, or a group across the mate boundary of a negative overlap: byte by byte
                for (uint32_t i = 0; i < 16u && k0 + i < len; i++) {
                    const uint32_t p = rc ? len - 1u - (k0 + i) : k0 + i;
                    const uint32_t q = qs[p];
                    uint32_t b = p < keep ? sa[p] : sb[p];
                    if (implied_n && q == nq) b = 'N';
                    if (rc) b = comp4_acgtn(b) & 0xFFu;
                    if (o.codes) b = code4_acgtn(b) & 0xFFu;
                    const uint32_t sh = 8u * (i & 3u), m = ~(0xFFu << sh);
                    wb[i >> 2] = (wb[i >> 2] & m) | (b << sh); wq[i >> 2] = (wq[i >> 2] & m) | (((q - o.qoff4) & 0xFFu) << sh);
                }
            }
        }
        store_group16(o.bases, o.quals, row * o.row_len + k0, o.row_len, k0, o.vec, wb, wq);
    }
}
