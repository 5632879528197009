// enc/rows_text.h - fixed-stride base / quality rows -> FASTQ text (rfq_rows_to_text, rfq_encode_rows): the way back from rfq_decode_rows
// Part of rfq_encode_kernels.h (included from there, last; not a stand-alone header).
#pragma once
// Row i is record i: name '\n' bases '\n' '+' '\n' quals '\n' - name_len + 2 * len + 5 bytes.  k_rows_sizes judges the lengths and the name offsets and
// writes the records' sizes (scanned to offsets by the host's scan_exclusive); k_rows_text writes the text.  For RFQ_PE_TWO_FILES the even rows make
// text 1 and the odd rows text 2: two size arrays, two scans, two launches of the writer (first = 0 / 1, step = 2).
#define RT_ERR_LEN     (1u << 0)      // a length that is negative or greater than row_len                       (RFQ_E_ARG)
#define RT_ERR_NOFF    (1u << 1)      // name offsets that decrease, or a last one past names_len                 (RFQ_E_ARG)
#define RT_ERR_LEN0    (1u << 2)      // a read of no bases                                                        (RFQ_E_DATA; all below too)
#define RT_ERR_NAME0   (1u << 3)      // a name of no bytes
#define RT_ERR_CODE    (1u << 4)      // writer: a base code above 4
#define RT_ERR_BASE    (1u << 5)      // writer: an ASCII base outside 0x21..0x7E
#define RT_ERR_QUAL    (1u << 6)      // writer: a quality character outside 0x21..0x7E
#define RT_ERR_NAMELB  (1u << 7)      // writer: '\n' or '\r' inside a name
struct RowsIn {
    const uint8_t* bases; const uint8_t* quals; const int32_t* lens;          // [n_rows][row_len], [n_rows][row_len], [n_rows]
    const uint8_t* names; const uint64_t* name_off;                           // the name lines back to back; [n_rows + 1] offsets into them
    uint64_t n_rows, names_len, row_len;
    uint32_t codes;                                                           // bases are codes A0 C1 G2 T3 N4
    uint32_t qoff, qoff4;                                                     // quality offset, and repeated in the four bytes of a word
    uint32_t vec;                                                             // row_len % 16 == 0 and both row buffers 16-byte aligned: rows are loaded in whole 16-byte groups
};
// what the host reads back: zeroed per call, bad_row = ~0
struct RowsStat { uint32_t err, pad; unsigned long long bad_row, n_bases; };

// grid ceil(n_rows / 256) x 256 threads, a thread per row
__global__ void __launch_bounds__(256) k_rows_sizes(RowsIn in, uint32_t two, uint64_t* __restrict__ sz0, uint64_t* __restrict__ sz1, RowsStat* __restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long nb = 0; uint32_t bad = 0;
    if (i < in.n_rows) {
        const int32_t len = in.lens[i]; const uint64_t a = in.name_off[i], b = in.name_off[i + 1];
        if (len < 0 || (uint64_t)(uint32_t)len > in.row_len) bad |= RT_ERR_LEN; else if (len == 0) bad |= RT_ERR_LEN0;
        if (b < a || (i + 1 == in.n_rows && b > in.names_len)) bad |= RT_ERR_NOFF; else if (b == a) bad |= RT_ERR_NAME0;
        const uint64_t rec = bad ? 0ull : (b - a) + 2ull * (uint32_t)len + 5ull;
        if (two) ((i & 1u) ? sz1 : sz0)[i >> 1] = rec; else sz0[i] = rec;
        if (!bad) nb = (uint32_t)len;
    }
    unsigned long long tot; (void)block_excl_sum<unsigned long long>(nb, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&st->n_bases, tot);
    if (bad) { atomicOr(&st->err, bad); atomicMin(&st->bad_row, (unsigned long long)i); }
}

// x + y in each byte, mod 256 (the reverse of dec/rows.h sub_bytes)
__device__ __forceinline__ uint32_t add_bytes(uint32_t x, uint32_t y) { return ((x & 0x7F7F7F7Fu) + (y & 0x7F7F7F7Fu)) ^ ((x ^ y) & 0x80808080u); }
// codes 0 1 2 3 4 -> A C G T N (the reverse of code4_acgtn): the code indexes a 5-entry table, four bytes in one v_perm_b32
__device__ __forceinline__ uint32_t ascii4_of_code(uint32_t w) { return __builtin_amdgcn_perm(0x0000004Eu, 0x54474341u, w & 0x07070707u); }
// 0x80 in every byte that is above 4 / outside 0x21..0x7E
__device__ __forceinline__ uint32_t bytes_gt4(uint32_t w) { return (((w & 0x7F7F7F7Fu) + 0x7B7B7B7Bu) | w) & 0x80808080u; }
__device__ __forceinline__ uint32_t bytes_not_graph(uint32_t w) { const uint32_t l = w & 0x7F7F7F7Fu; return (((l + 0x01010101u) | w) | ~(l + 0x5F5F5F5Fu)) & 0x80808080u; }
// 16 bytes at any byte address of a caller's buffer, and not a byte outside [p, p + 16).  rows in whole groups (RowsIn::vec): the one or two aligned
// 16-byte groups that hold them - both lie inside the row - and a funnel shift; otherwise one load of an align-1 type.
struct __attribute__((packed, aligned(1))) RtU16 { uint32_t a, b, c, d; };
__device__ __forceinline__ void rt_ld16(const uint8_t* p, bool groups, uint32_t (&w)[4]) {
    if (groups) {
        const uint4* a = (const uint4*)((uintptr_t)p & ~(uintptr_t)15); const uint32_t s = (uint32_t)((uintptr_t)p & 15u), sh = 8u * (s & 3u);
        const uint4 lo = a[0]; const uint4 hi = s ? a[1] : lo;
        switch (s >> 2) {
        case 0: w[0] = lds_funnel(lo.y, lo.x, sh); w[1] = lds_funnel(lo.z, lo.y, sh); w[2] = lds_funnel(lo.w, lo.z, sh); w[3] = lds_funnel(hi.x, lo.w, sh); break;
        case 1: w[0] = lds_funnel(lo.z, lo.y, sh); w[1] = lds_funnel(lo.w, lo.z, sh); w[2] = lds_funnel(hi.x, lo.w, sh); w[3] = lds_funnel(hi.y, hi.x, sh); break;
        case 2: w[0] = lds_funnel(lo.w, lo.z, sh); w[1] = lds_funnel(hi.x, lo.w, sh); w[2] = lds_funnel(hi.y, hi.x, sh); w[3] = lds_funnel(hi.z, hi.y, sh); break;
        default: w[0] = lds_funnel(hi.x, lo.w, sh); w[1] = lds_funnel(hi.y, hi.x, sh); w[2] = lds_funnel(hi.z, hi.y, sh); w[3] = lds_funnel(hi.w, hi.z, sh); break;
        }
    } else { const RtU16 v = *(const RtU16*)p; w[0] = v.a; w[1] = v.b; w[2] = v.c; w[3] = v.d; }
}

#define RT_TPB 256
#define RT_ITER 4
#define RT_TILE (RT_TPB * 16u * RT_ITER)      // text bytes of a workgroup: 16 KiB
#define RT_RECS (RT_TILE / 8u + 2u)           // a record has 8 bytes or more ("@\nA\n+\nI\n"): the one a tile starts in, those that start inside it, the end of the last
struct RtRec { uint64_t row, start, nl, size; uint32_t len; const uint8_t* name; const uint8_t* b; const uint8_t* q; };
__device__ __forceinline__ RtRec rt_rec(const RowsIn& in, uint64_t row, uint64_t start) {
    RtRec r; const uint64_t n0 = in.name_off[row];
    r.row = row; r.start = start; r.nl = in.name_off[row + 1] - n0; r.len = (uint32_t)in.lens[row]; r.size = r.nl + 2ull * r.len + 5ull;
    r.name = in.names + n0; r.b = in.bases + row * in.row_len; r.q = in.quals + row * in.row_len;
    return r;
}
// byte p of a record
__device__ __forceinline__ uint32_t rt_byte(const RowsIn& in, const RtRec& r, uint64_t p, uint32_t& bad) {
    if (p < r.nl) { const uint32_t c = r.name[p]; if (c == '\n' || c == '\r') bad |= RT_ERR_NAMELB; return c; }
    p -= r.nl;
    if (p == 0) return '\n';
    p -= 1;
    if (p < r.len) {
        uint32_t c = r.b[p];
        if (in.codes) { if (c > 4u) bad |= RT_ERR_CODE; c = ascii4_of_code(c) & 0xFFu; } else if (c < 0x21u || c > 0x7Eu) bad |= RT_ERR_BASE;
        return c;
    }
    p -= r.len;
    if (p < 3) return p == 1 ? '+' : '\n';
    p -= 3;
    if (p < r.len) { const uint32_t c = (r.q[p] + in.qoff) & 0xFFu; if (c < 0x21u || c > 0x7Eu) bad |= RT_ERR_QUAL; return c; }
    return '\n';
}
// grid ceil(N / RT_TILE) x 256 threads.  The work follows the OUTPUT: a workgroup owns RT_TILE bytes of the text - whole 16-byte groups of the (16-byte aligned)
// output buffer, whatever residue the records start at - and a thread one group at a time, consecutive threads consecutive groups: every store is an aligned
// 16-byte store and a wave's stores are one contiguous KiB.  Only the text's last group, where it is not whole, is written byte by byte.
// The records of a tile: thread 0 finds the one the tile starts in (binary search in off[], the exclusive scan of the record sizes, off[n_rec] = N), the
// offsets of the records behind it go to LDS, and every thread finds its group's record there.  A group that lies inside one name, base or quality line
// (most do: four line ends per record) is one 16-byte load at the source's own alignment, the transform on four words (v_perm for the codes, a byte-wise
// add for the quality offset) and the store; a group that holds a line end is put together byte by byte in registers.
// first / step: record k of this text is row first + k * step.
__global__ void __launch_bounds__(RT_TPB) k_rows_text(RowsIn in, const uint64_t* __restrict__ off, uint64_t n_rec, uint32_t first, uint32_t step,
                                                      uint8_t* __restrict__ out, uint64_t N, RowsStat* __restrict__ st) {
    __shared__ uint64_t s_off[RT_RECS + 1]; __shared__ uint64_t s_r0;
    const uint64_t A0 = (uint64_t)blockIdx.x * RT_TILE;
    if (threadIdx.x == 0) {
        uint64_t lo = 0, hi = n_rec;                                          // off[lo] <= A0 < off[hi]
        while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (off[mid] <= A0) lo = mid; else hi = mid; }
        s_r0 = lo;
    }
    __syncthreads();
    const uint64_t r0 = s_r0;
    for (uint32_t k = threadIdx.x; k <= RT_RECS; k += RT_TPB) s_off[k] = r0 + k <= n_rec ? off[r0 + k] : ~0ull;
    __syncthreads();
    uint32_t bad = 0; unsigned long long bad_row = ~0ull;
    for (uint32_t it = 0; it < RT_ITER; it++) {
        const uint64_t A = A0 + ((uint64_t)(it * RT_TPB + threadIdx.x) << 4);
        if (A >= N) break;
        uint32_t lo = 0, hi = RT_RECS;                                        // s_off[lo] <= A < s_off[hi]: records of 8 bytes or more put s_off[RT_RECS] behind the tile
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_off[mid] <= A) lo = mid; else hi = mid; }
        RtRec r = rt_rec(in, first + (r0 + lo) * step, s_off[lo]);
        uint64_t p = A - r.start;
        const bool whole = A + 16u <= N;
        uint32_t w[4]; bool done = false; uint32_t b = 0;
        if (whole) {
            if (p + 16u <= r.nl) {
                rt_ld16(r.name + p, false, w);
#pragma unroll
                for (int i = 0; i < 4; i++) if (eq_bytes_full(w[i], 0x0A0A0A0Au) | eq_bytes_full(w[i], 0x0D0D0D0Du)) b |= RT_ERR_NAMELB;
                done = true;
            } else if (p >= r.nl + 1u && p + 16u <= r.nl + 1u + r.len) {
                rt_ld16(r.b + (p - r.nl - 1u), in.vec != 0, w);
                if (in.codes) {
#pragma unroll
                    for (int i = 0; i < 4; i++) { if (bytes_gt4(w[i])) b |= RT_ERR_CODE; w[i] = ascii4_of_code(w[i]); }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) if (bytes_not_graph(w[i])) b |= RT_ERR_BASE;
                }
                done = true;
            } else if (p >= r.nl + r.len + 4u && p + 16u <= r.nl + 2ull * r.len + 4u) {
                rt_ld16(r.q + (p - r.nl - r.len - 4u), in.vec != 0, w);
#pragma unroll
                for (int i = 0; i < 4; i++) { w[i] = add_bytes(w[i], in.qoff4); if (bytes_not_graph(w[i])) b |= RT_ERR_QUAL; }
                done = true;
            }
            if (b && bad_row == ~0ull) bad_row = r.row;
        }
        if (!done) {
            // a group with a line end (or the text's last, short one): byte by byte, into two 64-bit halves
            unsigned long long h0 = 0, h1 = 0; uint32_t k = lo;
            const uint32_t n = whole ? 16u : (uint32_t)(N - A);
            for (uint32_t i = 0; i < n; i++) {
                if (p >= r.size) { k++; r = rt_rec(in, first + (r0 + k) * step, s_off[k]); p = 0; }
                const unsigned long long c = rt_byte(in, r, p, b); p++;
                if (b && bad_row == ~0ull) bad_row = r.row;
                if (i < 8u) h0 |= c << (8u * i); else h1 |= c << (8u * (i - 8u));
            }
            w[0] = (uint32_t)h0; w[1] = (uint32_t)(h0 >> 32); w[2] = (uint32_t)h1; w[3] = (uint32_t)(h1 >> 32);
        }
        bad |= b;
        if (whole) *(uint4*)(out + A) = make_uint4(w[0], w[1], w[2], w[3]);
        else {
            const unsigned long long h0 = ((unsigned long long)w[1] << 32) | w[0], h1 = ((unsigned long long)w[3] << 32) | w[2];
            for (uint32_t i = 0; i < (uint32_t)(N - A); i++) out[A + i] = (uint8_t)(i < 8u ? h0 >> (8u * i) : h1 >> (8u * (i - 8u)));
        }
    }
    if (bad) { atomicOr(&st->err, bad); atomicMin(&st->bad_row, bad_row); }
}
