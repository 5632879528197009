// enc/rows_judge.h - rows -> a verdict per row: a keep byte, a window (start, len), a reason byte and four metrics, in the arrays rfq_select_rows takes, and
// one QC summary of the batch (rfq_judge_rows): the step that DECIDES, between rfq_decode_rows / rfq_text_rows and rfq_select_rows
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose group reductions, 16-byte pieces and unit walk it uses; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the row bytes (include/rfq_hip.h has the rules).  A lane owns 16 consecutive positions of a row: one 16-byte load of the
// bases and one of the qualities, turned at once into 16-bit masks (is G, is N, below qual_q, >= 20, >= 30, differs from the byte before) by SWAR compares and
// v_dot4 - every count is a popcount of a mask under a span.  The qualities' running sums go to LDS (E[i] = the sum of the tile's first i qualities), so a window
// sum is two LDS reads and the three searches are min / max reductions over "my first / last start whose window is good / bad".
//   k_judge_rows<16> / <64>   the common path: a row of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) / by a wave; its bytes are loaded ONCE
//                             and every step runs on registers and LDS.  256 threads: 16 / 4 rows at a time, JR_ITER times.
//   k_judge_rows_long         any row length: a wave per row walks the row in tiles of `tile` window starts (1024; RFQ_JUDGE=general: 64, so that small rows
//                             have seams) with the cut window's halo behind them (tile + window - 1 <= 2047 bytes, two loads per lane), once per step.
// All sums are integers and leave a workgroup as JR_NSUM atomic adds: the result is the same bit for bit from run to run.
#define JR_NSUM 14                    // n_kept, why x 5, (bases, qsum, q20, q30) of the reads, the same of the kept windows
#define JR_ITER 8u
#define JR_CUT_FRONT 1u
#define JR_CUT_RIGHT 2u
#define JR_CUT_TAIL  4u
struct JudgeIn {
    const uint8_t* b; const uint8_t* q; const int32_t* lens;                  // b / q null: no base / quality criterion is set (the host saw to it); their counts are 0
    uint64_t total;                                                           // bytes of a row buffer: n_rows * row_len
    uint32_t n_rows, row_len;
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffers 16-byte aligned: a lane's group may be loaded whole
    uint32_t ascii;                                                           // bases are FASTQ bytes (N n, G g), else codes (4, 2)
    uint32_t trim_front, trim_tail, poly_g, cut_flags, cut_window, cut_mean_q, max_len, min_len;
    int32_t  max_n;
    uint32_t min_mean_q, qual_q, max_lowq_pct, min_complexity_pct;
    uint32_t tile;                                                            // k_judge_rows_long: window starts per tile (a multiple of 16, <= 1024)
    uint8_t* keep; int32_t* start; int32_t* len; uint8_t* why; uint32_t* metrics;   // [n_rows] each ([n_rows][4]), or null
};
typedef RowsSums<JR_NSUM> JudgeStat;

// ---- a lane's 16 bytes
__device__ __forceinline__ uint32_t jr_g_bits(const JudgeIn& in, const uint32_t (&b)[4]) {
    return in.ascii ? rows_eq_bits(b, 0xDFDFDFDFu, 0x47474747u) : rows_eq_bits(b, 0xFFFFFFFFu, 0x02020202u);
}
__device__ __forceinline__ uint32_t jr_n_bits(const JudgeIn& in, const uint32_t (&b)[4]) {
    return in.ascii ? rows_eq_bits(b, 0xDFDFDFDFu, 0x4E4E4E4Eu) : rows_eq_bits(b, 0xFFFFFFFFu, 0x04040404u);
}
// bit j: byte j differs from the byte in front of it (prev: the byte in front of byte 0)
__device__ __forceinline__ uint32_t jr_trans_bits(const uint32_t (&b)[4], uint32_t prev) {
    const uint32_t t[4] = { ~eq_bytes_full(b[0], (b[0] << 8) | (prev & 0xFFu)), ~eq_bytes_full(b[1], (b[1] << 8) | (b[0] >> 24)), ~eq_bytes_full(b[2], (b[2] << 8) | (b[1] >> 24)),
                            ~eq_bytes_full(b[3], (b[3] << 8) | (b[2] >> 24)) };
    return rows_bits(t);
}
// E[i] lives at word i + i / 16: the lanes of a group read and write 16 positions apart - 17 words, another bank each
__device__ __forceinline__ uint32_t jr_ix(uint32_t i) { return i + (i >> 4); }
// E[rel0 + j + 1] = base + q[0] + ... + q[j] for the lane's 16 qualities
__device__ __forceinline__ void jr_put(uint32_t* E, uint32_t rel0, uint32_t base, const uint32_t (&q)[4]) {
    uint32_t s = base;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) { s += (q[j >> 2] >> (8u * (j & 3u))) & 0xFFu; E[jr_ix(rel0 + j + 1u)] = s; }
}
// bit j: the window of w qualities that starts at the lane's position j is good - its sum is at least thr.  Only the starts in `valid` are looked at (the others'
// windows end behind what E holds).
__device__ __forceinline__ uint32_t jr_good(const uint32_t* E, uint32_t rel0, uint32_t w, unsigned long long thr, uint32_t valid) {
    uint32_t good = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
        if ((valid >> j) & 1u) { const uint32_t s = E[jr_ix(rel0 + j + w)] - E[jr_ix(rel0 + j)]; if ((unsigned long long)s >= thr) good |= 1u << j; }
    return good;
}
__device__ __forceinline__ uint32_t jr_first(uint32_t m, uint32_t x0) { return m ? x0 + (uint32_t)__ffs((int)m) - 1u : 0xFFFFFFFFu; }    // the first position in m; none: ~0
__device__ __forceinline__ uint32_t jr_last1(uint32_t m, uint32_t x0) { return m ? x0 + 32u - (uint32_t)__clz((int)m) : 0u; }              // the last position in m, + 1; none: 0

// the counts of a final window and the row's verdict
struct JrRow { uint32_t a, e; unsigned long long qsum, qsum_in; uint32_t n_cnt, lowq, trans, q20o, q30o, q20i, q30i, l; };
// One lane per row writes the row's outputs and adds it to the sums it keeps for the workgroup.
__device__ __forceinline__ void jr_verdict(const JudgeIn& in, uint64_t g, const JrRow& r, unsigned long long (&acc)[JR_NSUM]) {
    const unsigned long long n = r.e - r.a;
    uint32_t why = 0;
    if (n < in.min_len) why |= 1u;
    if (in.max_n >= 0 && r.n_cnt > (uint32_t)in.max_n) why |= 2u;
    if (r.qsum < (unsigned long long)in.min_mean_q * n) why |= 4u;
    if (in.qual_q > 0u && (unsigned long long)r.lowq * 100ull > (unsigned long long)in.max_lowq_pct * n) why |= 8u;
    if (n > 1ull && (unsigned long long)r.trans * 100ull < (unsigned long long)in.min_complexity_pct * (n - 1ull)) why |= 16u;
    if (in.keep) in.keep[g] = why ? 0u : 1u;
    if (in.start) in.start[g] = (int32_t)r.a;
    if (in.len) in.len[g] = (int32_t)n;
    if (in.why) in.why[g] = (uint8_t)why;
    if (in.metrics) { uint32_t* const m = in.metrics + 4ull * g; m[0] = (uint32_t)r.qsum; m[1] = r.n_cnt; m[2] = r.lowq; m[3] = r.trans; }
    acc[0] += why == 0u;
#pragma unroll
    for (int k = 0; k < 5; k++) acc[1 + k] += (why >> k) & 1u;
    acc[6] += r.l; acc[7] += r.qsum_in; acc[8] += r.q20i; acc[9] += r.q30i;
    if (why == 0u) { acc[10] += n; acc[11] += r.qsum; acc[12] += r.q20o; acc[13] += r.q30o; }
}

// grid ceil(n_rows / (256 / LPR * JR_ITER)) x 256 threads.  A group of the workgroup (UnitGroup: LPR lanes) judges a row per step, JR_ITER steps.  A group's E
// lives in the group's own part of the LDS, which only its wave touches: no barrier in the loop.  Steps are switched by kernel arguments (the same in
// every lane); what depends on the ROW - an empty window - only masks: the reductions are called by every lane of the wave in every step that is on.
template <int LPR> __global__ void __launch_bounds__(256) k_judge_rows(JudgeIn in, JudgeStat* __restrict__ st) {
    constexpr uint32_t T = LPR * 16u, ES = T + T / 16u + 1u;
    const UnitGroup<LPR> ug{};
    __shared__ uint32_t s_E[UnitGroup<LPR>::R * ES];
    uint32_t* const E = s_E + ug.grp * ES;
    unsigned long long acc[JR_NSUM] = {};
    const uint32_t cw = in.cut_window, kq = in.qual_q < 256u ? in.qual_q : 256u;
    for (uint32_t it = 0; it < JR_ITER; it++) {
        const uint64_t g = ug.unit(it, JR_ITER);
        if (ug.past(g, in.n_rows)) break;
        const bool live = g < in.n_rows;
        const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u;
        const uint64_t rowbase = g * in.row_len;
        uint32_t b[4] = { 0u, 0u, 0u, 0u }, q[4] = { 0u, 0u, 0u, 0u };
        if (ug.x0 < l) { if (in.b) rows_ld16(in.b, in.vec_in, in.total, rowbase, ug.x0, l, b); if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, ug.x0, l, q); }
        const uint32_t prev = wave_shr1(b[3] >> 24, 0u);                    // (a group's lane 0 never looks at it: position 0 has no byte in front)
        const uint32_t mG = jr_g_bits(in, b), mN = jr_n_bits(in, b), mT = jr_trans_bits(b, prev);
        const uint32_t m20 = rows_ge_bits(q, 20u), m30 = rows_ge_bits(q, 30u), mLow = in.qual_q ? ~rows_ge_bits(q, kq) & 0xFFFFu : 0u;
        const uint32_t s16 = rows_sum16(q), inc = grp_incl_sum<LPR>(s16);
        jr_put(E, ug.x0, inc - s16, q);
        if (ug.gl == 0u) E[0] = 0u;
        wave_lds_sync();
        uint32_t a = in.trim_front < l ? in.trim_front : l, e = l - (in.trim_tail < l ? in.trim_tail : l);
        if (e < a) e = a;
        if (in.poly_g) {
            const uint32_t last1 = grp_max<LPR>(jr_last1(~mG & rows_span(ug.x0, a, e), ug.x0));      // behind the last base of [a, e) that is no G
            const uint32_t r = e - (last1 > a ? last1 : a);
            if (r >= in.poly_g) e -= r;
        }
        if (in.cut_flags & JR_CUT_FRONT) {
            const uint32_t w = cw < e - a ? cw : e - a; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
            const uint32_t valid = e > a ? rows_span(ug.x0, a, e - w + 1u) : 0u;
            const uint32_t p = grp_min<LPR>(jr_first(jr_good(E, ug.x0, w, thr, valid), ug.x0));
            if (e > a) { if (p == 0xFFFFFFFFu) e = a; else a = p; }
        }
        if (in.cut_flags & JR_CUT_RIGHT) {
            const uint32_t w = cw < e - a ? cw : e - a; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
            const uint32_t valid = e > a ? rows_span(ug.x0, a, e - w + 1u) : 0u;
            const uint32_t p = grp_min<LPR>(jr_first(valid & ~jr_good(E, ug.x0, w, thr, valid), ug.x0));
            if (e > a && p != 0xFFFFFFFFu) e = p;
        }
        if (in.cut_flags & JR_CUT_TAIL) {
            const uint32_t w = cw < e - a ? cw : e - a; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
            const uint32_t valid = e > a ? rows_span(ug.x0, a, e - w + 1u) : 0u;
            const uint32_t p1 = grp_max<LPR>(jr_last1(jr_good(E, ug.x0, w, thr, valid), ug.x0));
            if (e > a) { if (p1 == 0u) e = a; else e = p1 - 1u + w; }
        }
        if (in.max_len && e - a > in.max_len) e = a + in.max_len;
        const uint32_t win = rows_span(ug.x0, a, e), all = rows_span(ug.x0, 0u, l);
        const unsigned long long c0 = (unsigned long long)__popc(mN & win) | ((unsigned long long)__popc(mLow & win) << 16) |
                                      ((unsigned long long)__popc(mT & rows_span(ug.x0, a + 1u, e)) << 32) | ((unsigned long long)__popc(m20 & win) << 48);
        const unsigned long long c1 = (unsigned long long)__popc(m30 & win) | ((unsigned long long)__popc(m20 & all) << 16) | ((unsigned long long)__popc(m30 & all) << 32);
        const unsigned long long t0 = grp_sum<LPR>(c0), t1 = grp_sum<LPR>(c1);
        if (ug.gl == 0u && live) {
            JrRow r; r.a = a; r.e = e; r.l = l; r.qsum = E[jr_ix(e)] - E[jr_ix(a)]; r.qsum_in = E[jr_ix(l)];
            r.n_cnt = (uint32_t)t0 & 0xFFFFu; r.lowq = (uint32_t)(t0 >> 16) & 0xFFFFu; r.trans = (uint32_t)(t0 >> 32) & 0xFFFFu; r.q20o = (uint32_t)(t0 >> 48);
            r.q30o = (uint32_t)t1 & 0xFFFFu; r.q20i = (uint32_t)(t1 >> 16) & 0xFFFFu; r.q30i = (uint32_t)(t1 >> 32) & 0xFFFFu;
            jr_verdict(in, g, r, acc);
        }
        wave_lds_sync();                                                     // (the next row's sums go where these were read)
    }
    rows_sums_out<4>(acc, st->c);
}

// ---- any row length
// E[i] = the sum of the qualities at [t0, t0 + i) for i in 0 .. 2048, of which positions >= hi count as 0: a lane loads the 16 bytes at t0 + x0 and those at
// t0 + 1024 + x0 where they lie in front of t0 + ext (ext: what the tile's windows reach, <= 2047).  Called by the whole wave.
__device__ __forceinline__ void jr_tile_sums(const JudgeIn& in, uint64_t rowbase, uint32_t t0, uint32_t ext, uint32_t hi, uint32_t x0, uint32_t* E) {
    uint32_t q0[4] = { 0u, 0u, 0u, 0u }, q1[4] = { 0u, 0u, 0u, 0u };
    if (x0 < ext && t0 + x0 < hi) rows_ld16(in.q, in.vec_in, in.total, rowbase, t0 + x0, hi, q0);
    if (1024u + x0 < ext && t0 + 1024u + x0 < hi) rows_ld16(in.q, in.vec_in, in.total, rowbase, t0 + 1024u + x0, hi, q1);
    const uint32_t s0 = rows_sum16(q0), s1 = rows_sum16(q1), i0 = wave_incl_sum(s0), i1 = wave_incl_sum(s1), tot0 = wave_last(i0);
    jr_put(E, x0, i0 - s0, q0); jr_put(E, 1024u + x0, tot0 + i1 - s1, q1);
    if (x0 == 0u) E[0] = 0u;
    wave_lds_sync();
}
// grid n_rows x 64 threads: a wave per row, everything about the row is the same in every lane.  Tiles lie on the multiples of `tile` from the row's start, so
// every load is a 16-byte group of the row as in the common path.  One walk over [0, l) for the read's own sums, one per step that is on - a search ends in
// the tile that finds -, one over the final window for its counts.
__global__ void __launch_bounds__(64) k_judge_rows_long(JudgeIn in, JudgeStat* __restrict__ st) {
    __shared__ uint32_t s_E[2048u + 128u + 1u];
    uint32_t* const E = s_E;
    const uint64_t g = blockIdx.x; const uint32_t x0 = 16u * threadIdx.x, T = in.tile, cw = in.cut_window, kq = in.qual_q < 256u ? in.qual_q : 256u;
    const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u);
    const uint64_t rowbase = g * in.row_len;
    const bool mine = x0 < T;                                                // (this lane holds window starts of a tile)
    unsigned long long acc[JR_NSUM] = {};
    JrRow r; r.l = l; r.qsum = r.qsum_in = 0ull; r.n_cnt = r.lowq = r.trans = r.q20o = r.q30o = r.q20i = r.q30i = 0u;
    if (in.q) for (uint32_t t0 = 0; t0 < l; t0 += T) {
        uint32_t q[4] = { 0u, 0u, 0u, 0u };
        if (mine && t0 + x0 < l) rows_ld16(in.q, in.vec_in, in.total, rowbase, t0 + x0, l, q);
        const uint32_t all = mine ? rows_span(t0 + x0, 0u, l) : 0u;
        const unsigned long long c = (unsigned long long)rows_sum16(q) | ((unsigned long long)__popc(rows_ge_bits(q, 20u) & all) << 32) |
                                     ((unsigned long long)__popc(rows_ge_bits(q, 30u) & all) << 48);
        const unsigned long long t = wave_sum<unsigned long long>(c);
        r.qsum_in += (uint32_t)t; r.q20i += (uint32_t)(t >> 32) & 0xFFFFu; r.q30i += (uint32_t)(t >> 48);
    }
    uint32_t a = in.trim_front < l ? in.trim_front : l, e = l - (in.trim_tail < l ? in.trim_tail : l);
    if (e < a) e = a;
    if (in.poly_g && e > a) {
        uint32_t last1 = 0u;
        for (uint32_t t0 = (e - 1u) / T * T, lo_t = a / T * T; ; t0 -= T) {
            uint32_t b[4] = { 0u, 0u, 0u, 0u };
            if (mine && t0 + x0 < e) rows_ld16(in.b, in.vec_in, in.total, rowbase, t0 + x0, e, b);
            last1 = wave_max(mine ? jr_last1(~jr_g_bits(in, b) & rows_span(t0 + x0, a, e), t0 + x0) : 0u);
            if (last1 || t0 == lo_t) break;
        }
        const uint32_t run = e - (last1 > a ? last1 : a);
        if (run >= in.poly_g) e -= run;
    }
    if ((in.cut_flags & JR_CUT_FRONT) && e > a) {
        const uint32_t w = cw < e - a ? cw : e - a, last = e - w; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
        uint32_t p = 0xFFFFFFFFu;
        for (uint32_t t0 = a / T * T; t0 <= last && p == 0xFFFFFFFFu; t0 += T) {
            jr_tile_sums(in, rowbase, t0, T + w - 1u, e, x0, E);
            const uint32_t valid = mine ? rows_span(t0 + x0, a, last + 1u) : 0u;
            p = wave_min(jr_first(jr_good(E, x0, w, thr, valid), t0 + x0));
            wave_lds_sync();
        }
        if (p == 0xFFFFFFFFu) e = a; else a = p;
    }
    if ((in.cut_flags & JR_CUT_RIGHT) && e > a) {
        const uint32_t w = cw < e - a ? cw : e - a, last = e - w; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
        uint32_t p = 0xFFFFFFFFu;
        for (uint32_t t0 = a / T * T; t0 <= last && p == 0xFFFFFFFFu; t0 += T) {
            jr_tile_sums(in, rowbase, t0, T + w - 1u, e, x0, E);
            const uint32_t valid = mine ? rows_span(t0 + x0, a, last + 1u) : 0u;
            p = wave_min(jr_first(valid & ~jr_good(E, x0, w, thr, valid), t0 + x0));
            wave_lds_sync();
        }
        if (p != 0xFFFFFFFFu) e = p;
    }
    if ((in.cut_flags & JR_CUT_TAIL) && e > a) {
        const uint32_t w = cw < e - a ? cw : e - a, last = e - w; const unsigned long long thr = (unsigned long long)in.cut_mean_q * w;
        uint32_t p1 = 0u;
        for (uint32_t t0 = last / T * T, lo_t = a / T * T; ; t0 -= T) {
            jr_tile_sums(in, rowbase, t0, T + w - 1u, e, x0, E);
            const uint32_t valid = mine ? rows_span(t0 + x0, a, last + 1u) : 0u;
            p1 = wave_max(jr_last1(jr_good(E, x0, w, thr, valid), t0 + x0));
            wave_lds_sync();
            if (p1 || t0 == lo_t) break;
        }
        if (p1 == 0u) e = a; else e = p1 - 1u + w;
    }
    if (in.max_len && e - a > in.max_len) e = a + in.max_len;
    if (e > a) for (uint32_t t0 = a / T * T; t0 < e; t0 += T) {
        uint32_t b[4] = { 0u, 0u, 0u, 0u }, q[4] = { 0u, 0u, 0u, 0u };
        const uint32_t p0 = t0 + x0; const bool on = mine && p0 < e;
        if (on) { if (in.b) rows_ld16(in.b, in.vec_in, in.total, rowbase, p0, e, b); if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, p0, e, q); }
        if (on && a > p0) {                                                  // (the qualities in front of the window do not count)
            const uint32_t f = a - p0 < 16u ? a - p0 : 16u;
#pragma unroll
            for (int i = 0; i < 4; i++) q[i] &= ~low_bytes((int)f - 4 * i);
        }
        uint32_t prev = wave_shr1(b[3] >> 24, 0u);
        if (threadIdx.x == 0u && in.b && p0 > a) prev = in.b[rowbase + p0 - 1u];      // (the tile in front holds it: a byte of the row, inside the window)
        const uint32_t win = on ? rows_span(p0, a, e) : 0u, mLow = in.qual_q ? ~rows_ge_bits(q, kq) & 0xFFFFu : 0u;
        const unsigned long long c0 = (unsigned long long)__popc(jr_n_bits(in, b) & win) | ((unsigned long long)__popc(mLow & win) << 16) |
                                      ((unsigned long long)__popc(on ? jr_trans_bits(b, prev) & rows_span(p0, a + 1u, e) : 0u) << 32) |
                                      ((unsigned long long)__popc(rows_ge_bits(q, 20u) & win) << 48);
        const unsigned long long c1 = (unsigned long long)__popc(rows_ge_bits(q, 30u) & win) | ((unsigned long long)rows_sum16(q) << 16);
        const unsigned long long u0 = wave_sum<unsigned long long>(c0), u1 = wave_sum<unsigned long long>(c1);
        r.n_cnt += (uint32_t)u0 & 0xFFFFu; r.lowq += (uint32_t)(u0 >> 16) & 0xFFFFu; r.trans += (uint32_t)(u0 >> 32) & 0xFFFFu; r.q20o += (uint32_t)(u0 >> 48);
        r.q30o += (uint32_t)u1 & 0xFFFFu; r.qsum += u1 >> 16;
    }
    r.a = a; r.e = e;
    if (threadIdx.x == 0u) jr_verdict(in, g, r, acc);
    rows_sums_out<1>(acc, st->c);
}
