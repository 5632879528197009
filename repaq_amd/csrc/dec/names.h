// dec/names.h - the name lines alone (rfq_decode_names): their lengths and offsets, then the bytes
// Part of rfq_decode_kernels.h (included from there, in order; not a stand-alone header).
#pragma once
// ---- names (name re-assembly src/rfqcodec.cpp:1157-1231): name = name1 piece + ":lane:tile:x:y" (the parts the header has) + name2 piece, as k_dec_emit writes
// it in front of a record - without the read table, the quality / base streams and the overlap table the records need.  Two kernels behind k_dec_coords:
//   k_dec_namelen   a workgroup per chunk: every read's name bytes, their CHUNK-LOCAL exclusive prefix (one entry more than the chunk has reads: its total, so
//                   chunk c's entries sit at [rbase + c, rbase + c + reads]), the prefixes of the per-read name1 / name2 pieces where a chunk stores them per
//                   read, the chunk's total as 64 bits for one small scan over the chunks
//   k_dec_names     a workgroup per run of consecutive reads of one chunk, a thread per read: the names of a tile composed in LDS and stored in aligned
//                   16-byte groups, name_off[row] = range base + chunk base + local prefix beside them
// Both take a read's lengths from nm_parts: the same bytes of the image through the same function, so the writer cannot disagree with the offsets.  The
// middle's digits never pass through HBM: the lengths kernel counts them, the writer formats them (mid_put).
#define NM_READS 256u             // reads of a tile: one per thread
#define NM_OCAP 16384u            // output tile bytes: 256 names of up to 63 bytes on average; a tile of longer names goes byte-wise straight to global memory
#define NM_MIDROW 40u             // ":255:65535:4294967295:4294967295" is 32 bytes; mid_put's 8-byte store may run seven bytes past a part
__device__ __forceinline__ uint32_t nm_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
struct NmParts { DName m; uint32_t k, len; };                       // k: bytes of the middle; len = n1 + k + n2
__device__ __forceinline__ NmParts nm_parts(const uint8_t* cp, const DChunk& d, const DevHeader* D, const uint32_t* xv, const uint32_t* yv, uint32_t r) {
    NmParts p; p.m = dec_name_parts(cp, d, D, xv, yv, r);
    const uint32_t hf = D->flags; uint32_t k = 0;
    if (hf & H_LANE) k += 1u + nm_digits(p.m.lane);
    if (hf & H_TILE) k += 1u + nm_digits(p.m.tile);
    if (hf & H_X) k += 1u + nm_digits(p.m.x);
    if (hf & H_Y) k += 1u + nm_digits(p.m.y);
    p.k = k; p.len = p.m.n1 + k + p.m.n2;
    return p;
}
// npl[rbase + c + r]: name bytes of chunk c in front of its read r (entry `reads`: the chunk's total); ppl (null where no chunk of the range stores pieces per read):
// x / y = bytes of the per-read name1 / name2 pieces in front of read r; ctot[c]: the chunk's name bytes.  st->list_need <- the largest chunk total (a chunk of 4 GiB
// of names and more does not fit the 32-bit local prefixes: the host refuses it), st->max_one <- the longest name.
__global__ void __launch_bounds__(256) k_dec_namelen(const uint8_t* __restrict__ img, const DChunk* __restrict__ CH, const DevHeader* __restrict__ D,
                                                     const uint32_t* __restrict__ xv, const uint32_t* __restrict__ yv, uint32_t* __restrict__ npl, uint2* __restrict__ ppl,
                                                     unsigned long long* __restrict__ ctot, DecStatus* st) {
    const uint32_t c = blockIdx.x; const DChunk d = CH[c]; const uint8_t* cp = img + d.off; const uint32_t fl = d.flags, hf = D->flags;
    const size_t fp = (size_t)d.rbase + c;
    unsigned long long carry = 0; uint32_t c1 = 0, c2 = 0, mx = 0;
    for (uint32_t r0 = 0; r0 < d.reads; r0 += blockDim.x) {             // block-uniform
        const uint32_t r = r0 + threadIdx.x; U4 v; v.a = v.b = v.c = v.d = 0;
        if (r < d.reads) {
            const NmParts p = nm_parts(cp, d, D, xv, yv, r);
            v.a = p.len; v.b = (fl & C_NAME1_SAME) ? 0u : p.m.n1; v.c = (!(hf & H_NAME2) || (fl & C_NAME2_SAME)) ? 0u : p.m.n2;
            if (p.len > mx) mx = p.len;
        }
        U4 tot; const U4 ex = block_excl_sum<U4>(v, &tot);
        if (r < d.reads) { npl[fp + r] = (uint32_t)carry + ex.a; if (ppl) ppl[fp + r] = make_uint2(c1 + ex.b, c2 + ex.c); }
        carry += tot.a; c1 += tot.b; c2 += tot.c;
    }
    mx = wave_max(mx);
    if (lane_id() == 0 && mx) atomicMax(&st->max_one, mx);
    if (threadIdx.x == 0) { npl[fp + d.reads] = (uint32_t)carry; ctot[c] = carry; atomicMax(&st->list_need, carry); }
}
// where the names go: names[base + ...] (any alignment), off[row] (row = the read's index in the image); end = the blob's bytes (nothing is written at or behind it)
struct NamesOut { uint8_t* names; uint64_t* off; uint64_t base, end; };
// byte i of a name piece that starts `at` bytes into its section [sec, sec + size) of the chunk at image offset `coff`: '?' outside the section or the image
__device__ __forceinline__ uint8_t nm_src(const uint8_t* __restrict__ img, uint64_t img_bytes, uint64_t coff, uint32_t sec, uint32_t size, uint64_t at) {
    const uint64_t g = coff + sec + at;
    return (at < size && g < img_bytes) ? img[g] : (uint8_t)'?';
}
__global__ void __launch_bounds__(256) k_dec_names(const uint8_t* __restrict__ img, uint64_t img_bytes, const DChunk* __restrict__ CH, const DevHeader* __restrict__ D,
                                                   const uint32_t* __restrict__ xv, const uint32_t* __restrict__ yv, const uint32_t* __restrict__ npl,
                                                   const uint2* __restrict__ ppl, const unsigned long long* __restrict__ cbase, NamesOut o, uint32_t n_chunks) {
    __shared__ uint4 s_out4[NM_OCAP / 16 + 2];
    __shared__ unsigned long long s_mid[NM_READS * NM_MIDROW / 8];      // a 40-byte row per thread
    __shared__ uint8_t s_n1[256], s_n2[256];                            // the chunk's one copy of a shared name1 / name2
    const uint32_t c = blockIdx.y; const DChunk d = CH[c]; const uint8_t* cp = img + d.off;
    const uint32_t fl = d.flags, hf = D->flags, tid = threadIdx.x; const bool il = (fl & C_PE_INTERLEAVED) != 0;
    const uint32_t dpos = D->name2_diff_pos, dch = D->name2_diff_char;
    const bool same1 = (fl & C_NAME1_SAME) != 0, same2 = (fl & C_NAME2_SAME) != 0;
    const size_t fp = (size_t)d.rbase + c;
    const uint32_t per = (d.reads + gridDim.x - 1) / gridDim.x;
    const uint32_t rs = blockIdx.x * per, re = rs + per < d.reads ? rs + per : d.reads;
    if (rs >= re) return;                                               // block-uniform
    // the blob may start anywhere: positions count from the 16-byte boundary at or below it, so that an aligned position is an aligned address
    const uint32_t sh = (uint32_t)((uintptr_t)o.names & 15u); uint8_t* const nb = o.names - sh;
    const uint64_t cb = o.base + cbase[c];                              // the chunk's first name byte in the blob
    if (tid < 255u) {
        s_n1[tid] = same1 ? nm_src(img, img_bytes, d.off, d.o_n1, d.n1_size, tid) : (uint8_t)0;
        s_n2[tid] = (same2 && (hf & H_NAME2)) ? nm_src(img, img_bytes, d.off, d.o_n2, d.n2_size, tid) : (uint8_t)0;
    }
    if (blockIdx.x == 0 && c + 1 == n_chunks && tid == 0) o.off[(size_t)d.rbase_abs + d.reads] = cb + npl[fp + d.reads];     // (the next range, if any, writes the same value)
    __syncthreads();
    for (uint32_t cur = rs; cur < re; cur += NM_READS) {                // block-uniform
        const uint32_t r = cur + tid, last = cur + NM_READS < re ? cur + NM_READS : re;
        const uint32_t t0 = npl[fp + cur], bytes = npl[fp + last] - t0;  // the tile's names: bytes [t0, t0 + bytes) of the chunk's
        const bool tiled = bytes + 16u <= NM_OCAP;
        const uint64_t gbeg = cb + t0 + sh;                             // (position from nb)
        if (r < re) {
            const NmParts p = nm_parts(cp, d, D, xv, yv, r);
            const uint32_t my = npl[fp + r] - t0;
            // what this name may write: its own bytes, inside the tile's, inside the blob (the lengths kernel computed all three from the same bytes)
            uint32_t lim = my < bytes ? bytes - my : 0u; if (p.len < lim) lim = p.len;
            { const uint64_t at = cb + t0 + my; const uint64_t room = at < o.end ? o.end - at : 0ull; if (room < lim) lim = (uint32_t)room; }
            uint8_t* const row = (uint8_t*)(s_mid + (NM_MIDROW / 8u) * tid);
            { uint32_t k = 0;
              if (hf & H_LANE) k += mid_put(row, k, NM_MIDROW, p.m.lane);
              if (hf & H_TILE) k += mid_put(row, k, NM_MIDROW, p.m.tile);
              if (hf & H_X) k += mid_put(row, k, NM_MIDROW, p.m.x);
              if (hf & H_Y) k += mid_put(row, k, NM_MIDROW, p.m.y); }
            uint8_t* const w = tiled ? (uint8_t*)s_out4 + (uint32_t)(gbeg & 15ull) + my : nb + gbeg + my;
            const uint2 pp = ppl ? ppl[fp + r] : make_uint2(0u, 0u);
            const bool patch = same2 && il && (r & 1u) && dch != 0;
            uint32_t q = 0;
            for (uint32_t i = 0; i < p.m.n1 && q < lim; i++, q++) w[q] = same1 ? s_n1[i] : nm_src(img, img_bytes, d.off, d.o_n1, d.n1_size, (uint64_t)pp.x + i);
            for (uint32_t i = 0; i < p.k && q < lim; i++, q++) w[q] = row[i];
            for (uint32_t i = 0; i < p.m.n2 && q < lim; i++, q++)
                w[q] = (patch && i == dpos) ? (uint8_t)dch : (same2 ? s_n2[i] : nm_src(img, img_bytes, d.off, d.o_n2, d.n2_size, (uint64_t)pp.y + i));
            o.off[(size_t)d.rbase_abs + r] = cb + t0 + my;
        }
        __syncthreads();
        if (tiled) { const uint64_t gend = gbeg + bytes, cap = o.end + sh; flush_span(s_out4, nb, gbeg, gend < cap ? gend : cap); }
        __syncthreads();                                                // (the next tile's names go into the same rows)
    }
}
