// enc/rows_lanes.h - what the kernels of the rows family share: the reductions over a group of lanes, a lane's 16 bytes of a row as SWAR masks, and the walk, length
// check, candidate test and sums of the calls that DECIDE (rfq_judge_rows, rfq_adapter_rows, rfq_dedup_rows, rfq_profile_rows, rfq_screen_rows, rfq_kmers_rows,
// rfq_demux_rows: a verdict or a count per unit - a row, or a pair of rows -, no row moved).
// Part of rfq_encode_kernels.h (included from there, in front of the rows_*.h that use it; not a stand-alone header).  What only the calls that read bases 2 bits
// at a time share - a lane's classes, the k-mers of a row, the set of slots - is rows_kmer_lanes.h's.
#pragma once
#define ROWS_ERR_LEN 1u               // a length that is negative or greater than row_len (RFQ_E_ARG)
// what the host reads back of a deciding call: zeroed per call, bad_row = ~0, N sums of the call's own
template <int N> struct RowsSums { uint32_t err, pad; unsigned long long bad_row; unsigned long long c[N]; };

// ---- reductions over a group of LPR lanes (16: a DPP row; 64: the wave), the result in every lane of the group.  Called by ALL lanes of the wave.
#ifdef RFQ_SIMT_EMULATION
template <class T> __device__ __forceinline__ T row_incl_sum(T v) {
    const int l = lane_id() & 15;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) { T t = __shfl_up(v, (unsigned)d); if (l >= d) v = t + v; }
    return v;
}
template <class T> __device__ __forceinline__ T row_sum(T v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t row_min(uint32_t v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) { const uint32_t t = __shfl_xor(v, d); if (t < v) v = t; }
    return v;
}
__device__ __forceinline__ uint32_t row_max(uint32_t v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) { const uint32_t t = __shfl_xor(v, d); if (t > v) v = t; }
    return v;
}
#else
// row_shr:1/2/4/8 - the scan of RFQ_DPP_SCAN without its two steps across the rows; row_ror:1/2/4/8 - after them every lane holds its row's 16 values combined
#define RFQ_DPP_ROW_ALL(v, OP) { RFQ_DPP_STEP(v, OP, v, 0x121, 0xF) RFQ_DPP_STEP(v, OP, v, 0x122, 0xF) RFQ_DPP_STEP(v, OP, v, 0x124, 0xF) RFQ_DPP_STEP(v, OP, v, 0x128, 0xF) }
template <class T> __device__ __forceinline__ T row_incl_sum(T v) {
    RFQ_DPP_STEP(v, RFQ_OP_ADD, T(), 0x111, 0xF) RFQ_DPP_STEP(v, RFQ_OP_ADD, T(), 0x112, 0xF) RFQ_DPP_STEP(v, RFQ_OP_ADD, T(), 0x114, 0xF) RFQ_DPP_STEP(v, RFQ_OP_ADD, T(), 0x118, 0xF)
    return v;
}
template <class T> __device__ __forceinline__ T row_sum(T v) { RFQ_DPP_ROW_ALL(v, RFQ_OP_ADD) return v; }
__device__ __forceinline__ uint32_t row_min(uint32_t v) { RFQ_DPP_ROW_ALL(v, RFQ_OP_MIN) return v; }
__device__ __forceinline__ uint32_t row_max(uint32_t v) { RFQ_DPP_ROW_ALL(v, RFQ_OP_MAX) return v; }
#endif
template <int LPR, class T> __device__ __forceinline__ T grp_incl_sum(T v) { if constexpr (LPR == 16) return row_incl_sum(v); else return wave_incl_sum(v); }
template <int LPR, class T> __device__ __forceinline__ T grp_sum(T v) { if constexpr (LPR == 16) return row_sum(v); else return wave_sum(v); }
template <int LPR> __device__ __forceinline__ uint32_t grp_min(uint32_t v) { if constexpr (LPR == 16) return row_min(v); else return wave_min(v); }
template <int LPR> __device__ __forceinline__ uint32_t grp_max(uint32_t v) { if constexpr (LPR == 16) return row_max(v); else return wave_max(v); }

// ---- a lane's 16 bytes
// 0x80 in every byte of w that is >= k (k in 0 .. 256; bytes are unsigned)
__device__ __forceinline__ uint32_t rows_ge(uint32_t w, uint32_t k) {
    const uint32_t lo = w & 0x7F7F7F7Fu;
    return k <= 128u ? ((lo + (128u - k) * 0x01010101u) | w) & 0x80808080u : ((lo + (256u - k) * 0x01010101u) & w) & 0x80808080u;
}
// bit j = the 0x80 flag of byte j of the 16 bytes
__device__ __forceinline__ uint32_t rows_bits(const uint32_t (&t)[4]) {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) m |= udot4((t[i] >> 7) & 0x01010101u, 0x08040201u, 0u) << (4 * i);
    return m;
}
__device__ __forceinline__ uint32_t rows_ge_bits(const uint32_t (&q)[4], uint32_t k) {
    const uint32_t t[4] = { rows_ge(q[0], k), rows_ge(q[1], k), rows_ge(q[2], k), rows_ge(q[3], k) };
    return rows_bits(t);
}
__device__ __forceinline__ uint32_t rows_eq_bits(const uint32_t (&b)[4], uint32_t fold, uint32_t pat) {
    const uint32_t t[4] = { eq_bytes_full(b[0] & fold, pat), eq_bytes_full(b[1] & fold, pat), eq_bytes_full(b[2] & fold, pat), eq_bytes_full(b[3] & fold, pat) };
    return rows_bits(t);
}
// bit j: position x0 + j lies in [lo, hi)
__device__ __forceinline__ uint32_t rows_span(uint32_t x0, uint32_t lo, uint32_t hi) {
    if (hi <= lo || hi <= x0 || lo >= x0 + 16u) return 0u;
    const uint32_t f = lo > x0 ? lo - x0 : 0u, t = hi - x0 < 16u ? hi - x0 : 16u;
    return ((1u << t) - 1u) & ~((1u << f) - 1u);
}
__device__ __forceinline__ uint32_t rows_sum16(const uint32_t (&q)[4]) { return udot4(q[3], 0x01010101u, udot4(q[2], 0x01010101u, udot4(q[1], 0x01010101u, udot4(q[0], 0x01010101u, 0u)))); }
// Bytes [off, off + 16) of the row that starts at byte `rowbase` of buf (off a multiple of 16, off < lim <= row_len): bytes at positions >= lim come back 0.
// Never a byte outside the buffer: whole aligned groups lie inside their row; else 16 bytes at the row's own alignment wherever they still lie inside the
// buffer; only at the buffer's very end byte by byte.
__device__ __forceinline__ void rows_ld16(const uint8_t* buf, uint32_t vec_in, uint64_t total, uint64_t rowbase, uint32_t off, uint32_t lim, uint32_t (&w)[4]) {
    const uint64_t p = rowbase + off; const uint32_t have = lim - off < 16u ? lim - off : 16u;
    if (vec_in) rt_ld16(buf + p, true, w);
    else if (p + 16u <= total) rt_ld16(buf + p, false, w);
    else {
        w[0] = w[1] = w[2] = w[3] = 0u;
        for (uint32_t i = 0; i < have; i++) w[i >> 2] |= (uint32_t)buf[p + i] << (8u * (i & 3u));
    }
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] &= low_bytes((int)have - 4 * i);
}

// ---- a row's length, of a call's *In block (lens, row_len): lens[g] where it is a length, else 0 (nothing of such a row is read)
template <class In> __device__ __forceinline__ uint32_t rows_len_or0(const In& in, uint64_t g) {
    const int32_t l = in.lens[g];
    return (l >= 0 && (uint32_t)l <= in.row_len) ? (uint32_t)l : 0u;
}
// the same, and a bad length is reported (by the lanes that say `first`: one per row is enough): the call is refused with the first such row
template <class In, class Stat> __device__ __forceinline__ uint32_t rows_len_checked(const In& in, uint64_t g, Stat* st, bool first) {
    const int32_t l = in.lens[g];
    if (l >= 0 && (uint32_t)l <= in.row_len) return (uint32_t)l;
    if (first) { atomicOr(&st->err, ROWS_ERR_LEN); atomicMin(&st->bad_row, (unsigned long long)g); }
    return 0u;
}
// The workgroup's sums: a reduction per wave, one atomic add per sum that is not 0, into dst[0 .. N).  Every thread of the workgroup (NW waves) calls it.
template <int NW, int N> __device__ __forceinline__ void rows_sums_out(unsigned long long (&acc)[N], unsigned long long* dst) {
    __shared__ unsigned long long s_red[NW][N];
#pragma unroll
    for (int k = 0; k < N; k++) { const unsigned long long t = wave_sum<unsigned long long>(acc[k]); if (lane_id() == 0) s_red[wave_id()][k] = t; }
    if constexpr (NW > 1) __syncthreads(); else wave_lds_sync();
    if (threadIdx.x < (uint32_t)N) {
        unsigned long long t = 0;
        for (int w = 0; w < NW; w++) t += s_red[w][threadIdx.x];
        if (t) atomicAdd(&dst[threadIdx.x], t);
    }
}

// ---- the walk of a common-path kernel: 256 threads in groups of LPR lanes, a group takes a unit (a row, or the pair of rows 2u and 2u + 1) per step
__device__ __forceinline__ uint64_t rows_unit_row(uint32_t pairs, uint64_t u, uint32_t i) { return pairs ? 2ull * u + i : u; }
// unit u is a candidate, of a call's *In block (cand: a byte per ROW, null = every unit; pairs): all of its rows are
template <class In> __device__ __forceinline__ bool rows_cand(const In& in, uint64_t u) {
    if (!in.cand) return true;
    return in.pairs ? (in.cand[2ull * u] != 0u && in.cand[2ull * u + 1ull] != 0u) : in.cand[u] != 0u;
}
// A thread's place: group `grp` of the workgroup's R, lane `gl` of the group, which holds the row's bytes from x0 on.  A wave holds GW groups.
template <int LPR> struct UnitGroup {
    static constexpr uint32_t R = 256u / LPR, GW = 64u / LPR;
    const uint32_t grp = threadIdx.x / LPR, gl = threadIdx.x % LPR, x0 = 16u * gl;
    __device__ __forceinline__ uint64_t unit(uint32_t it, uint32_t iter) const { return unit_of(blockIdx.x, it, iter); }
    // the same for a workgroup that is the blk-th of its kind (rfq_profile_rows: the workgroups of a mate count among themselves)
    __device__ __forceinline__ uint64_t unit_of(uint32_t blk, uint32_t it, uint32_t iter) const { return ((uint64_t)blk * iter + it) * R + grp; }
    // the wave's FIRST unit lies behind the last one - the same in every lane of the wave, so a loop may end on it with wave-wide reductions in its body
    __device__ __forceinline__ bool past(uint64_t u, uint64_t n_units) const { return u - grp % GW >= n_units; }
};
