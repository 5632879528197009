// enc/rows_adapter.h - rows -> the length adapter removal leaves of every row, the detector that cut it, the insert size and mismatch count of every pair's
// overlap, one summary and an insert-size histogram (rfq_adapter_rows): the step in front of rfq_judge_rows.  It decides and moves no bytes.
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose 16-byte pieces and unit walk it uses; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the base bytes (include/rfq_hip.h has the rules).  A read becomes three bit planes of 64 positions per word: H and L, the two
// bits of its class (A 0, C 1, G 2, T 3), and V, "is one of A C G T and lies inside the read".  A lane turns its 16 bytes into three 16-bit masks by SWAR compares
// and v_dot4 (rows_lanes.h's pieces) and stores them as 16-bit pieces of the words in LDS.  The reverse complement of R2 is the same masks bit-reversed, stored in
// reverse lane order, H and L inverted: position j of y lies at bit T - l2 + j of its planes (T: the bits a group holds), between NW words of zeros on either side -
// so "y shifted by d against x" is one funnel of two neighbouring words per plane at bit 2T - insert, the same for every word of x.  Agreement is
// ~((Hx ^ Hy) | (Lx ^ Ly)) & Vx & Vy: V is 0 outside either read, so no span mask is needed and ov(d) is plain arithmetic; diff = ov - popcount.  A lane takes a
// shift (an order index), a group a block of LPR of them; the first acceptable one is a min-reduction over the order index and the group stops behind the first
// block that holds one.  The adapter match is the same primitive with the adapter's two planes (64 bases: one word each) in the kernel arguments, a lane per position.
//   k_adapter_rows<16> / <64>  the common path: a unit (a pair, or a row without pairs) of rows of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) /
//                              by a wave.  256 threads: 16 / 4 units at a time, AR_ITER times.
//   k_adapter_rows_any         any row length (and every one with RFQ_ADAPTER=general): a wave per unit, a lane per shift / position, the bytes compared one by one
//                              from the rows themselves.  QUADRATIC in the read length like the rule itself, and with no bit planes to shorten it: slow on very long rows.
// All sums are integers and leave a workgroup as AR_NSUM atomic adds, the histogram is integer atomic adds: the result is the same bit for bit from run to run.
#define AR_NSUM 6                     // pairs_found, rows_cut, rows_cut_overlap, rows_cut_adapter, bases_in, bases_out
#define AR_ITER 4u
#define AR_NONE 0xFFFFFFFFu
struct AdapterIn {
    const uint8_t* b; const int32_t* lens;
    uint64_t total;                                                           // bytes of the row buffer: n_rows * row_len
    uint32_t n_rows, n_units, row_len;                                        // units: pairs (rows 2u, 2u + 1) or single rows
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffer 16-byte aligned: a lane's group may be loaded whole
    uint32_t ascii, pairs;
    uint32_t min_overlap, max_diff, max_diff_pct;
    unsigned long long a_h[2], a_l[2]; uint32_t a_m[2];                       // the adapters' class planes (base j at bit j) and lengths; 0: off.  [1] is the odd rows' (pairs)
    uint32_t adapter_min, adapter_mm_per, hist_len;
    int32_t* len; uint8_t* how; int32_t* insert; int32_t* diff; unsigned long long* hist;     // [n_rows], [n_rows], [n_units], [n_units], [hist_len], or null
};
typedef RowsSums<AR_NSUM> AdapterStat;
typedef uint16_t __attribute__((may_alias)) ar_u16;                           // a lane's 16 positions of a plane word

// ---- the rules
__device__ __forceinline__ bool ar_overlap_ok(const AdapterIn& in, uint32_t ov, uint32_t diff) {
    return ov >= in.min_overlap && diff <= in.max_diff && (unsigned long long)diff * 100ull <= (unsigned long long)in.max_diff_pct * ov;
}
__device__ __forceinline__ bool ar_adapter_ok(const AdapterIn& in, uint32_t c, uint32_t diff) {
    return c >= in.adapter_min && (in.adapter_mm_per ? (unsigned long long)diff * in.adapter_mm_per <= (unsigned long long)c : diff == 0u);
}
// shifts in the order they are tried: n0 of them from 0 upwards, then -1, -2, ...
__device__ __forceinline__ uint32_t ar_n_up(const AdapterIn& in, uint32_t l1) { return l1 >= in.min_overlap ? l1 - in.min_overlap + 1u : 0u; }
__device__ __forceinline__ uint32_t ar_n_down(const AdapterIn& in, uint32_t l2) { return l2 > in.min_overlap ? l2 - in.min_overlap : 0u; }
__device__ __forceinline__ int32_t ar_shift(uint32_t k, uint32_t n0) { return k < n0 ? (int32_t)k : -(int32_t)(k - n0 + 1u); }
__device__ __forceinline__ uint32_t ar_ov(int32_t d, uint32_t l1, uint32_t l2) {
    const int64_t lo = d > 0 ? d : 0, e2 = (int64_t)l2 + d, hi = e2 < (int64_t)l1 ? e2 : (int64_t)l1;
    return hi > lo ? (uint32_t)(hi - lo) : 0u;
}
// a unit's verdict: its rows' lengths and adapter cuts, the overlap's insert (-1: none) and mismatches
struct ArUnit { uint32_t l[2], cut_a[2]; int32_t insert; uint32_t diff; };
// One lane per unit writes the unit's outputs and adds it to the sums it keeps for the workgroup.
__device__ __forceinline__ void ar_result(const AdapterIn& in, uint64_t u, const ArUnit& r, unsigned long long (&acc)[AR_NSUM]) {
    const uint32_t nr = in.pairs ? 2u : 1u;
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        const uint32_t l = r.l[i], cut_o = (r.insert >= 0 && (uint32_t)r.insert < l) ? (uint32_t)r.insert : l, cut_a = r.cut_a[i];
        const uint32_t n = cut_o < cut_a ? cut_o : cut_a, how = (cut_o < l ? 1u : 0u) | (cut_a < l ? 2u : 0u);
        if (in.len) in.len[g] = (int32_t)n;
        if (in.how) in.how[g] = (uint8_t)how;
        acc[1] += how != 0u; acc[2] += how & 1u; acc[3] += how >> 1; acc[4] += l; acc[5] += n;
    }
    if (in.pairs) {
        if (in.insert) in.insert[u] = r.insert;
        if (in.diff) in.diff[u] = (int32_t)r.diff;
        if (r.insert >= 0) {
            acc[0] += 1ull;
            if (in.hist) atomicAdd(&in.hist[(uint32_t)r.insert < in.hist_len - 1u ? (uint32_t)r.insert : in.hist_len - 1u], 1ull);
        }
    }
}

// ---- a lane's 16 bytes as three 16-bit masks
// bit j = bit 0 of byte j of the 16 bytes
__device__ __forceinline__ uint32_t ar_bit0s(const uint32_t (&t)[4]) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) m |= udot4(t[i] & 0x01010101u, 0x08040201u, 0u) << (4 * i);
    return m;
}
struct ArBits { uint32_t h, l, v; };
// Case-folded, bit 2 of a base letter is the class's high bit and bit 1 ^ bit 2 its low bit (A 0x41, C 0x43, G 0x47, T 0x54); a code is its class.  h and l of a
// position that is not in v are not looked at.  span: the lane's positions inside the read (a byte of 0 behind a read is code A).
__device__ __forceinline__ ArBits ar_bits(uint32_t ascii, const uint32_t (&b)[4], uint32_t span) {
    uint32_t th[4], tl[4], tv[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (ascii) {
            const uint32_t f = b[i] & 0xDFDFDFDFu;
            th[i] = f >> 2; tl[i] = (f >> 1) ^ (f >> 2);
            tv[i] = eq_bytes_full(f, 0x41414141u) | eq_bytes_full(f, 0x43434343u) | eq_bytes_full(f, 0x47474747u) | eq_bytes_full(f, 0x54545454u);
        } else { th[i] = b[i] >> 1; tl[i] = b[i]; tv[i] = ~rows_ge(b[i], 4u) >> 7; }
    }
    ArBits r; r.h = ar_bit0s(th); r.l = ar_bit0s(tl); r.v = ar_bit0s(tv) & span;
    return r;
}
// the 16 bits of m in reverse order
#ifdef RFQ_SIMT_EMULATION
__device__ __forceinline__ uint32_t ar_rev16(uint32_t m) {
    m = ((m >> 1) & 0x5555u) | ((m & 0x5555u) << 1); m = ((m >> 2) & 0x3333u) | ((m & 0x3333u) << 2); m = ((m >> 4) & 0x0F0Fu) | ((m & 0x0F0Fu) << 4);
    return ((m >> 8) | (m << 8)) & 0xFFFFu;
}
#else
__device__ __forceinline__ uint32_t ar_rev16(uint32_t m) { return __brev(m) >> 16; }      // v_bfrev_b32
#endif
// bits [sh, sh + 64) of the 128 bits hi:lo (sh < 64)
__device__ __forceinline__ unsigned long long ar_funnel(unsigned long long lo, unsigned long long hi, uint32_t sh) { return (lo >> sh) | ((hi << 1) << (63u - sh)); }

// The smallest acceptable position of adapter `ai` in the read of l bases whose planes are P (H, L, V: FW words each, the last one 0), or l.  Called by ALL lanes of
// the wave (the loop ends for the whole wave at once; a group that is done only masks).
template <int LPR> __device__ __forceinline__ uint32_t ar_adapter_cut(const AdapterIn& in, const unsigned long long* P, uint32_t FW, uint32_t l, uint32_t ai, uint32_t gl) {
    const uint32_t m = in.a_m[ai];
    if (!m) return l;                                                        // (a kernel argument: the same in every lane)
    const unsigned long long AH = in.a_h[ai], AL = in.a_l[ai], mask = m >= 64u ? ~0ull : (1ull << m) - 1ull;
    uint32_t best = AR_NONE;
    for (uint32_t k0 = 0; ; k0 += (uint32_t)LPR) {
        const bool act = best == AR_NONE && k0 < l;
        if (!__any(act)) break;
        uint32_t cand = AR_NONE; const uint32_t p = k0 + gl;
        if (act && p < l) {
            const uint32_t wi = p >> 6, sh = p & 63u, c = m < l - p ? m : l - p;
            const unsigned long long h = ar_funnel(P[wi], P[wi + 1u], sh), lo = ar_funnel(P[FW + wi], P[FW + wi + 1u], sh), v = ar_funnel(P[2u * FW + wi], P[2u * FW + wi + 1u], sh);
            const unsigned long long agree = ~((h ^ AH) | (lo ^ AL)) & v & mask;      // (v is 0 from the read's end on: at most c bits)
            if (ar_adapter_ok(in, c, c - (uint32_t)__popcll(agree))) cand = p;
        }
        const uint32_t mn = grp_min<LPR>(cand);
        if (act) best = mn;
    }
    return best == AR_NONE ? l : best;
}

// grid ceil(n_units / (256 / LPR * AR_ITER)) x 256 threads.  A group of the workgroup (UnitGroup: LPR lanes) takes a unit per step, AR_ITER steps.  A group's planes
// live in the group's own part of the LDS, which only its wave touches: no barrier in the loop.  Per group: the forward planes of both rows, F[row][H L V][NW + 1]
// (the word behind them stays 0: the adapter's funnel reads it), and the planes of y, Y[H L V][3 NW + 1], y's T bits in words NW .. 2 NW - 1 and zeros around
// them.  The zeros are written once; every step rewrites all T bits of every plane it uses.
template <int LPR> __global__ void __launch_bounds__(256) k_adapter_rows(AdapterIn in, AdapterStat* __restrict__ st) {
    constexpr uint32_t T = LPR * 16u, NW = T / 64u, FW = NW + 1u, YW = 3u * NW + 1u, GS = 6u * FW + 3u * YW;
    const UnitGroup<LPR> ug{};
    __shared__ unsigned long long s_P[UnitGroup<LPR>::R * GS];
    unsigned long long* const F = s_P + ug.grp * GS; unsigned long long* const Y = F + 6u * FW;
    for (uint32_t i = ug.gl; i < GS; i += (uint32_t)LPR) F[i] = 0ull;
    wave_lds_sync();
    unsigned long long acc[AR_NSUM] = {};
    const uint32_t nr = in.pairs ? 2u : 1u;
    for (uint32_t it = 0; it < AR_ITER; it++) {
        const uint64_t u = ug.unit(it, AR_ITER);
        if (ug.past(u, in.n_units)) break;
        const bool live = u < in.n_units;
        const uint64_t g0 = rows_unit_row(in.pairs, u, 0u);
        ArUnit r; r.l[0] = r.l[1] = 0u; r.cut_a[0] = r.cut_a[1] = 0u; r.insert = -1; r.diff = 0u;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t l = live ? rows_len_checked(in, g0 + i, st, ug.gl == 0u) : 0u;
            r.l[i] = l;
            uint32_t b[4] = { 0u, 0u, 0u, 0u };
            if (ug.x0 < l) rows_ld16(in.b, in.vec_in, in.total, (g0 + i) * in.row_len, ug.x0, l, b);
            const ArBits m = ar_bits(in.ascii, b, rows_span(ug.x0, 0u, l));
            unsigned long long* const P = F + 3u * i * FW;
            ((ar_u16*)P)[ug.gl] = (uint16_t)m.h; ((ar_u16*)(P + FW))[ug.gl] = (uint16_t)m.l; ((ar_u16*)(P + 2u * FW))[ug.gl] = (uint16_t)m.v;
            if (i == 1u) {                                                   // y = the reverse complement of R2: position j at bit T - l2 + j
                const uint32_t s = (uint32_t)LPR - 1u - ug.gl;
                ((ar_u16*)(Y + NW))[s] = (uint16_t)ar_rev16(m.h ^ 0xFFFFu); ((ar_u16*)(Y + YW + NW))[s] = (uint16_t)ar_rev16(m.l ^ 0xFFFFu);
                ((ar_u16*)(Y + 2u * YW + NW))[s] = (uint16_t)ar_rev16(m.v);
            }
        }
        wave_lds_sync();
        if (in.pairs) {
            const uint32_t l1 = r.l[0], l2 = r.l[1], n0 = ar_n_up(in, l1), nsh = n0 + ar_n_down(in, l2);
            uint32_t best = AR_NONE;                                         // (order index << 11) | diff: an index is below 2 T <= 2048, a diff at most T <= 1024
            for (uint32_t k0 = 0; ; k0 += (uint32_t)LPR) {
                const bool act = best == AR_NONE && k0 < nsh;
                if (!__any(act)) break;
                uint32_t cand = AR_NONE; const uint32_t k = k0 + ug.gl;
                if (act && k < nsh) {
                    const int32_t d = ar_shift(k, n0);
                    const uint32_t ov = ar_ov(d, l1, l2);
                    if (ov >= in.min_overlap) {
                        const uint32_t lo = d > 0 ? (uint32_t)d : 0u, w0 = lo >> 6, w1 = (lo + ov - 1u) >> 6;      // x positions [lo, lo + ov) are compared
                        const uint32_t at = 2u * T - (uint32_t)(d + (int32_t)l2), sh = at & 63u;                   // x position i meets bit i + at of Y
                        uint32_t wi = (at >> 6) + w0, cnt = 0u;
                        unsigned long long h0 = Y[wi], q0 = Y[YW + wi], v0 = Y[2u * YW + wi];
                        for (uint32_t w = w0; w <= w1; w++) {
                            wi++;
                            const unsigned long long h1 = Y[wi], q1 = Y[YW + wi], v1 = Y[2u * YW + wi];
                            const unsigned long long yh = ar_funnel(h0, h1, sh), yl = ar_funnel(q0, q1, sh), yv = ar_funnel(v0, v1, sh);
                            cnt += (uint32_t)__popcll(~((F[w] ^ yh) | (F[FW + w] ^ yl)) & F[2u * FW + w] & yv);
                            h0 = h1; q0 = q1; v0 = v1;
                        }
                        if (ar_overlap_ok(in, ov, ov - cnt)) cand = (k << 11) | (ov - cnt);
                    }
                }
                const uint32_t mn = grp_min<LPR>(cand);
                if (act) best = mn;
            }
            if (best != AR_NONE) { r.insert = ar_shift(best >> 11, n0) + (int32_t)l2; r.diff = best & 0x7FFu; }
        }
        for (uint32_t i = 0; i < nr; i++) r.cut_a[i] = ar_adapter_cut<LPR>(in, F + 3u * i * FW, FW, r.l[i], i, ug.gl);
        if (ug.gl == 0u && live) ar_result(in, u, r, acc);
        wave_lds_sync();                                                     // (the next unit's planes go where these were read)
    }
    rows_sums_out<4>(acc, st->c);
}

// ---- any row length
// class of a base byte: 0 .. 3 = A C G T, 4 = other
__device__ __forceinline__ uint32_t ar_cls(uint32_t ascii, uint8_t c) {
    if (!ascii) return c < 4u ? c : 4u;
    switch (c & 0xDFu) { case 0x41: return 0u; case 0x43: return 1u; case 0x47: return 2u; case 0x54: return 3u; default: return 4u; }
}
// grid n_units x 64 threads: a wave per unit, a lane per shift / position in blocks of 64, the bytes of the compared positions read one by one - only bytes
// in front of a read's length, so never outside the rows.  The first block that holds an acceptable shift ends the search.
__global__ void __launch_bounds__(64) k_adapter_rows_any(AdapterIn in, AdapterStat* __restrict__ st) {
    const uint64_t u = blockIdx.x; const uint32_t lane = threadIdx.x, nr = in.pairs ? 2u : 1u;
    const uint64_t g0 = rows_unit_row(in.pairs, u, 0u);
    unsigned long long acc[AR_NSUM] = {};
    ArUnit r; r.l[0] = r.l[1] = 0u; r.cut_a[0] = r.cut_a[1] = 0u; r.insert = -1; r.diff = 0u;
    for (uint32_t i = 0; i < nr; i++) r.l[i] = rows_len_checked(in, g0 + i, st, lane == 0u);
    if (in.pairs) {
        const uint8_t* const x = in.b + g0 * in.row_len; const uint8_t* const r2 = x + in.row_len;
        const uint32_t l1 = r.l[0], l2 = r.l[1], n0 = ar_n_up(in, l1), nsh = n0 + ar_n_down(in, l2);
        unsigned long long best = ~0ull;                                    // (order index << 32) | diff
        for (uint32_t k0 = 0; k0 < nsh && best == ~0ull; k0 += 64u) {
            unsigned long long cand = ~0ull; const uint32_t k = k0 + lane;
            if (k < nsh) {
                const int32_t d = ar_shift(k, n0);
                const uint32_t ov = ar_ov(d, l1, l2);
                if (ov >= in.min_overlap) {
                    const uint32_t j0 = d < 0 ? (uint32_t)-d : 0u;            // y positions [j0, j0 + ov) against x positions j + d
                    uint32_t diff = 0u;
                    for (uint32_t j = j0; j < j0 + ov; j++) {
                        const uint32_t cx = ar_cls(in.ascii, x[(uint32_t)((int32_t)j + d)]), cy = ar_cls(in.ascii, r2[l2 - 1u - j]);
                        diff += (cx > 3u || cy > 3u || cx != 3u - cy) ? 1u : 0u;
                    }
                    if (ar_overlap_ok(in, ov, diff)) cand = ((unsigned long long)k << 32) | diff;
                }
            }
            best = wave_min<unsigned long long>(cand);
            if (nsh - k0 <= 64u) break;                                     // (k0 + 64 may not fit 32 bits behind the last block)
        }
        if (best != ~0ull) { r.insert = ar_shift((uint32_t)(best >> 32), n0) + (int32_t)l2; r.diff = (uint32_t)best; }
    }
    for (uint32_t i = 0; i < nr; i++) {
        const uint32_t l = r.l[i], m = in.a_m[i];
        r.cut_a[i] = l;
        if (!m) continue;
        const uint8_t* const x = in.b + (g0 + i) * in.row_len;
        const unsigned long long AH = in.a_h[i], AL = in.a_l[i];
        for (uint32_t k0 = 0; k0 < l; k0 += 64u) {
            uint32_t cand = AR_NONE; const uint32_t p = k0 + lane;
            if (p < l) {
                const uint32_t c = m < l - p ? m : l - p;
                uint32_t diff = 0u;
                for (uint32_t j = 0; j < c; j++) diff += ar_cls(in.ascii, x[p + j]) != ((uint32_t)((AH >> j) & 1ull) << 1 | (uint32_t)((AL >> j) & 1ull)) ? 1u : 0u;
                if (ar_adapter_ok(in, c, diff)) cand = p;
            }
            const uint32_t mn = wave_min<uint32_t>(cand);
            if (mn != AR_NONE) { r.cut_a[i] = mn; break; }
        }
    }
    if (lane == 0u) ar_result(in, u, r, acc);
    rows_sums_out<1>(acc, st->c);
}
