// enc/rows_profile.h - rows under a keep byte and a window (start, len) per row -> the tables a QC report is built from: base content and score sum per cycle and
// class, the position x score distribution, the distributions of read length, per-read mean score and per-read GC content, and one summary per mate
// (rfq_profile_rows): the REPORT beside the steps that decide (rfq_judge_rows, rfq_adapter_rows, rfq_dedup_rows) and the ones that move (rfq_select_rows).
// Part of rfq_encode_kernels.h (included from there, last, behind rows_lanes.h whose 16-byte pieces, group reductions, unit walk and sums it uses; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the row bytes (include/rfq_hip.h has the rules).  A lane owns 16 consecutive positions of a row: one 16-byte load of the bases
// and one of the scores, the classes as one byte per position (SWAR), the window as a 16-bit span - the summary's counts are popcounts of masks under that span.
//   k_profile_rows<16> / <64>   the common path: a row of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) / by a wave.  A workgroup keeps ITS tables
//                               in dynamic LDS, adds to them with LDS atomics and flushes them once at its end: one 64-bit global atomicAdd per cell that is not 0.
//                               The flush is what a workgroup costs (150 cycles x (5 + 42) cells: about 7,000 adds), so the grid is a few workgroups per compute unit
//                               and the host hands in how many steps each takes (ProfileIn::steps).  With pairs a workgroup takes the rows of ONE mate (the even
//                               workgroups read 1, the odd ones read 2): its tables are one mate's, half the LDS, twice the resident workgroups.
//   k_profile_rows_long         any row length, any `cycles`, tables of any size (and every call with RFQ_PROFILE=general, in tiles of 64 positions so that small rows
//                               have seams): a wave per row walks the window in tiles of `tile` positions and adds straight to the tables in global memory.
// LDS layout (32-bit words; ProfileIn::o_* are the host's offsets, a table that is not asked for takes no room):
//   base   [CS][5] 64-bit cells  count << 32 | score sum of a cycle and class - ONE LDS atomic per position serves d_base_cnt and d_base_qsum
//   qh     [CS][QS] 32-bit cells position x score, QS = qbins | 1
//   len [len_bins], mq [qbins], gc [101] 32-bit cells
// CS = 16 * CH cycle slots, CH = ceil(cycles / 16), and cycle c lives in slot (c & 15) * CH + (c >> 4): the lanes of a group hold cycles 16 apart, which are
// NEIGHBOURING slots - 10 words apart in base, QS (odd) words apart in qh: another bank for each of the group's lanes.  The four groups of a <16> wave would hit the
// same cycles at once (windows mostly start at 0): group k walks its 16 positions from word k & 3 on, so that in one instruction the groups stand 4 cycles apart
// and same-address adds within a wave instruction are left to rows whose windows differ.  (A table per group does not fit; counts formed across the groups with
// ballots cost 80 ballots a step for four rows.)
// No overflow: a workgroup sees at most PF_ROWS_MAX = 2^24 rows (the host caps steps * R there and grows the grid instead), a cycle of a row adds at most 1 to a
// count and 255 to a score sum: 2^24 * 255 < 2^32, so neither half of a base cell carries into the other and no 32-bit cell wraps.
// No LDS index out of range, by construction (the interpreter build keeps LDS in host thread-local memory, where a sanitizer sees no overrun): the cycle is
// clamped to cycles - 1 < CS before pf_slot, the class is 0 .. 4 from pf_classes, the score bin is clamped to qbins - 1 < QS, the length bin to len_bins - 1, the
// GC percentage is at most 100, and the host refuses to launch with tables that exceed PF_LDS_MAX bytes (it takes the long kernel then).
#define PF_NSUM 16                    // per mate m, at 7 * m: counted, bases, qsum, q20, q30, gc, other; [14] max_len (an atomicMax); [15] ~(the first row with a bad window) (an atomicMax; 0: none)
#define PF_ERR_WIN 2u                 // a window that is negative or ends behind its read (RFQ_E_ARG); beside ROWS_ERR_LEN
#define PF_ROWS_MAX (1u << 24)        // rows a workgroup of the common path sees at most
#define PF_LDS_MAX (159u * 1024u)     // bytes of dynamic LDS a workgroup's tables may take (160 KiB a compute unit; rows_sums_out keeps 512 bytes of its own)
#define PF_WG_PER_CU 3u               // workgroups per compute unit the common path's grid is capped at
#define PF_GC_BINS 101u
static_assert((unsigned long long)PF_ROWS_MAX * 255ull < (1ull << 32), "a 32-bit LDS cell holds a workgroup's largest score sum");
static_assert(PF_LDS_MAX + 1024u <= 160u * 1024u, "the tables and the sums' block fit a compute unit's LDS");
struct ProfileIn {
    const uint8_t* b; const uint8_t* q; const int32_t* lens;                  // b / q null: the summary's base / score fields stay 0 (tables that need them: refused on the host)
    const uint8_t* keep; const int32_t* start; const int32_t* len;            // rfq_select_rows' triple; null: every row / 0 / to the end of the read
    uint64_t total;                                                           // bytes of a row buffer: n_rows * row_len
    uint32_t n_rows, row_len;
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffers 16-byte aligned: a lane's group may be loaded whole
    uint32_t ascii, pairs;
    uint32_t cycles, qbins, len_bins;
    uint32_t steps;                                                           // common path: steps of a workgroup (steps * R <= PF_ROWS_MAX)
    uint32_t tile;                                                            // k_profile_rows_long: positions per tile (a multiple of 16, <= 1024)
    uint32_t ch, qs;                                                          // common path: CH and QS of the LDS layout
    uint32_t o_base, o_qh, o_len, o_mq, o_gc, lds_words;                      // common path: the tables' first words (o_base is even), all words
    unsigned long long* base_cnt; unsigned long long* base_qsum; unsigned long long* qual_hist;       // [M][cycles][5], [M][cycles][5], [M][cycles][qbins], or null
    unsigned long long* len_hist; unsigned long long* meanq_hist; unsigned long long* gc_hist;        // [M][len_bins], [M][qbins], [M][101], or null
};
typedef RowsSums<PF_NSUM> ProfileStat;

// ---- a lane's 16 bytes
// the class of each base byte as a byte 0 .. 4 (rfq_adapter_rows' classes: code 0 .. 3 or A C G T in either case; 4: everything else)
__device__ __forceinline__ void pf_classes(uint32_t ascii, const uint32_t (&b)[4], uint32_t (&cls)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (ascii) {
            const uint32_t f = b[i] & 0xDFDFDFDFu;
            const uint32_t eA = eq_bytes_full(f, 0x41414141u), eC = eq_bytes_full(f, 0x43434343u), eG = eq_bytes_full(f, 0x47474747u), eT = eq_bytes_full(f, 0x54545454u);
            cls[i] = (eC & 0x01010101u) | (eG & 0x02020202u) | (eT & 0x03030303u) | (~(eA | eC | eG | eT) & 0x04040404u);
        } else {
            const uint32_t ge = rows_ge(b[i], 4u);                           // 0x80 in every byte that is 4 or more
            cls[i] = (b[i] & ~((ge >> 7) * 0xFFu)) | (ge >> 5);
        }
    }
}
// bit j: class 1 or 2 (bit 1 of class + 1; no byte carries: a class is at most 4) / class 4
__device__ __forceinline__ uint32_t pf_gc_bits(const uint32_t (&cls)[4]) {
    const uint32_t t[4] = { ((cls[0] + 0x01010101u) << 6) & 0x80808080u, ((cls[1] + 0x01010101u) << 6) & 0x80808080u, ((cls[2] + 0x01010101u) << 6) & 0x80808080u,
                            ((cls[3] + 0x01010101u) << 6) & 0x80808080u };
    return rows_bits(t);
}
__device__ __forceinline__ uint32_t pf_other_bits(const uint32_t (&cls)[4]) {
    const uint32_t t[4] = { (cls[0] << 5) & 0x80808080u, (cls[1] << 5) & 0x80808080u, (cls[2] << 5) & 0x80808080u, (cls[3] << 5) & 0x80808080u };
    return rows_bits(t);
}
// the scores at positions in front of the window do not count (p0: the lane's first position; those behind it come back 0 from rows_ld16)
__device__ __forceinline__ void pf_cut_front(uint32_t (&q)[4], uint32_t p0, uint32_t a) {
    if (a <= p0) return;
    const uint32_t f = a - p0 < 16u ? a - p0 : 16u;
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] &= ~low_bytes((int)f - 4 * i);
}
// the slot of cycle c (c < cycles <= 16 * ch)
__device__ __forceinline__ uint32_t pf_slot(uint32_t c, uint32_t ch) { return (c & 15u) * ch + (c >> 4); }
__device__ __forceinline__ uint32_t pf_slot_cycle(uint32_t s, uint32_t ch) { return (s % ch) * 16u + s / ch; }

// ---- a row's window
// [a, a + n) of row g of l bases (l: rows_len_checked's), and whether the row is counted.  A bad window is reported (by the lanes that say `first`) and comes back
// empty; a row whose LENGTH was bad has been reported already and is not looked at again.  Every row is judged, counted or not.
struct PfRow { uint32_t a, n; bool counted; };
__device__ __forceinline__ PfRow pf_window(const ProfileIn& in, uint64_t g, uint32_t l, ProfileStat* st, bool first) {
    PfRow r; r.a = 0u; r.n = 0u; r.counted = !in.keep || in.keep[g] != 0u;
    const int32_t lr = in.lens[g];
    if (lr < 0 || (uint32_t)lr > in.row_len) { r.counted = false; return r; }
    const long long s = in.start ? (long long)in.start[g] : 0ll, m = in.len ? (long long)in.len[g] : (long long)l - s;
    if (s < 0 || m < 0 || s + m > (long long)l) {
        if (first) { atomicOr(&st->err, PF_ERR_WIN); atomicMax(&st->c[15], ~(unsigned long long)g); }
        r.counted = false;
        return r;
    }
    r.a = (uint32_t)s; r.n = (uint32_t)m;
    return r;
}
// what a lane adds up for the summary of its mate
struct PfAcc { unsigned long long counted, bases, qsum, q20, q30, gc, other; uint32_t max_len; };
// a lane's 16 positions under `win` into its sums; returns qsum | acgt << 20 | gc << 32 of them for the row's totals (a row of the common path: <= 1024 positions)
__device__ __forceinline__ unsigned long long pf_lane_sums(const ProfileIn& in, const uint32_t (&cls)[4], const uint32_t (&q)[4], uint32_t win, PfAcc& acc) {
    const uint32_t s16 = rows_sum16(q), nw = (uint32_t)__popc(win);
    const uint32_t oth = in.b ? (uint32_t)__popc(pf_other_bits(cls) & win) : 0u, gc = in.b ? (uint32_t)__popc(pf_gc_bits(cls) & win) : 0u, acgt = in.b ? nw - oth : 0u;
    acc.bases += nw; acc.qsum += s16; acc.q20 += (uint32_t)__popc(rows_ge_bits(q, 20u) & win); acc.q30 += (uint32_t)__popc(rows_ge_bits(q, 30u) & win);
    acc.gc += gc; acc.other += oth;
    return (unsigned long long)s16 | ((unsigned long long)acgt << 20) | ((unsigned long long)gc << 32);
}
// the bins of a counted row of n positions with score sum qs, acgt positions of class 0 .. 3 and gc of class 1 or 2 (~0: the row is in no bin of that table)
__device__ __forceinline__ uint32_t pf_len_bin(const ProfileIn& in, uint32_t n) { return n < in.len_bins - 1u ? n : in.len_bins - 1u; }
__device__ __forceinline__ uint32_t pf_mq_bin(const ProfileIn& in, uint32_t n, unsigned long long qs) {
    if (!n) return 0xFFFFFFFFu;
    const unsigned long long m = qs / n;
    return m < in.qbins - 1u ? (uint32_t)m : in.qbins - 1u;
}
__device__ __forceinline__ uint32_t pf_gc_bin(unsigned long long acgt, unsigned long long gc) { return acgt ? (uint32_t)(100ull * gc / acgt) : 0xFFFFFFFFu; }      // (gc <= acgt: at most 100)
// The workgroup's sums: a lane's PfAcc at its mate's place.  Every thread of the workgroup (NW waves) calls it.
template <int NW> __device__ __forceinline__ void pf_sums_out(const PfAcc& a, uint32_t mate, ProfileStat* st) {
    const unsigned long long v[7] = { a.counted, a.bases, a.qsum, a.q20, a.q30, a.gc, a.other };
    unsigned long long acc[PF_NSUM] = {};
#pragma unroll
    for (int k = 0; k < 7; k++) { acc[k] = mate ? 0ull : v[k]; acc[7 + k] = mate ? v[k] : 0ull; }
    rows_sums_out<NW>(acc, st->c);
    const uint32_t mx = wave_max<uint32_t>(a.max_len);
    if (lane_id() == 0 && mx) atomicMax(&st->c[14], (unsigned long long)mx);
}

// grid (workgroups per mate) x (1 + pairs) x 256 threads; dynamic LDS: in.lds_words words.  A group of the workgroup (UnitGroup: LPR lanes) takes a row per step,
// in.steps steps.  What depends on the ROW only masks: the group reduction is called by every lane of the wave in every step.
template <int LPR> __global__ void __launch_bounds__(256) k_profile_rows(ProfileIn in, ProfileStat* __restrict__ st) {
    // (declared in 64-bit words: the base cells' alignment.  The interpreter's buffer for dynamic LDS holds 64 KB; there the tables get a block of their own, of
    // the size the host never exceeds)
#ifdef RFQ_SIMT_EMULATION
    __shared__ unsigned long long pf_lds64[PF_LDS_MAX / 8u];
#else
    RFQ_DYN_SHARED(unsigned long long, pf_lds64);
#endif
    uint32_t* const pf_lds = (uint32_t*)pf_lds64;
    const UnitGroup<LPR> ug{};
    const uint32_t mate = in.pairs ? blockIdx.x & 1u : 0u, blk = in.pairs ? blockIdx.x >> 1 : blockIdx.x;
    const uint64_t n_units = in.pairs ? in.n_rows / 2u : in.n_rows;
    for (uint32_t i = threadIdx.x; i < in.lds_words; i += 256u) pf_lds[i] = 0u;
    __syncthreads();
    unsigned long long* const t_base = (unsigned long long*)(pf_lds + in.o_base);
    uint32_t* const t_qh = pf_lds + in.o_qh; uint32_t* const t_len = pf_lds + in.o_len; uint32_t* const t_mq = pf_lds + in.o_mq; uint32_t* const t_gc = pf_lds + in.o_gc;
    const bool want_base = in.base_cnt || in.base_qsum, want_qh = in.qual_hist != nullptr;      // (kernel arguments: the same in every lane)
    const uint32_t rot = LPR == 16 ? ug.grp & 3u : 0u;                      // the word this group's walk over its 16 positions begins at
    PfAcc acc = {};
    for (uint32_t it = 0; it < in.steps; it++) {
        const uint64_t u = ug.unit_of(blk, it, in.steps);
        if (ug.past(u, n_units)) break;
        const bool live = u < n_units;
        const uint64_t g = in.pairs ? 2ull * u + mate : u;
        const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u;
        PfRow r; r.a = r.n = 0u; r.counted = false;
        if (live) r = pf_window(in, g, l, st, ug.gl == 0u);
        const uint32_t a = r.a, e = r.a + r.n;
        const uint64_t rowbase = g * in.row_len;
        uint32_t b[4] = { 0u, 0u, 0u, 0u }, q[4] = { 0u, 0u, 0u, 0u }, cls[4];
        const uint32_t win = r.counted ? rows_span(ug.x0, a, e) : 0u;
        if (win) { if (in.b) rows_ld16(in.b, in.vec_in, in.total, rowbase, ug.x0, e, b); if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, ug.x0, e, q); }
        pf_cut_front(q, ug.x0, a);
        pf_classes(in.ascii, b, cls);
        const unsigned long long t = grp_sum<LPR>(pf_lane_sums(in, cls, q, win, acc));
        if (ug.gl == 0u && r.counted) {
            const unsigned long long qs = t & 0xFFFFFull, acgt = (t >> 20) & 0xFFFull, gc = t >> 32;
            acc.counted += 1ull; acc.max_len = r.n > acc.max_len ? r.n : acc.max_len;
            if (in.len_hist) atomicAdd(&t_len[pf_len_bin(in, r.n)], 1u);
            const uint32_t mb = pf_mq_bin(in, r.n, qs), gb = pf_gc_bin(acgt, gc);
            if (in.meanq_hist && mb != 0xFFFFFFFFu) atomicAdd(&t_mq[mb], 1u);
            if (in.gc_hist && gb != 0xFFFFFFFFu) atomicAdd(&t_gc[gb < PF_GC_BINS ? gb : PF_GC_BINS - 1u], 1u);
        }
        if ((want_base || want_qh) && win) {
            // word i of the walk is word (i + rot) & 3 of the lane's 16 positions: the words change places, the positions keep their cycles
            if (rot & 1u) { uint32_t x = cls[0]; cls[0] = cls[1]; cls[1] = cls[2]; cls[2] = cls[3]; cls[3] = x; x = q[0]; q[0] = q[1]; q[1] = q[2]; q[2] = q[3]; q[3] = x; }
            if (rot & 2u) { uint32_t x = cls[0]; cls[0] = cls[2]; cls[2] = x; x = cls[1]; cls[1] = cls[3]; cls[3] = x; x = q[0]; q[0] = q[2]; q[2] = x; x = q[1]; q[1] = q[3]; q[3] = x; }
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t j0 = 4u * ((i + rot) & 3u);
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    if (!((win >> (j0 + k)) & 1u)) continue;
                    uint32_t c = ug.x0 + j0 + k - a;                        // the cycle is computed from the position and the window's start, never taken from the lane
                    c = c < in.cycles - 1u ? c : in.cycles - 1u;
                    const uint32_t s = pf_slot(c, in.ch), kc = (cls[i] >> (8u * k)) & 7u, qq = (q[i] >> (8u * k)) & 0xFFu;
                    if (want_base) atomicAdd(&t_base[s * 5u + (kc < 4u ? kc : 4u)], (1ull << 32) | (unsigned long long)qq);
                    if (want_qh) atomicAdd(&t_qh[s * in.qs + (qq < in.qbins - 1u ? qq : in.qbins - 1u)], 1u);
                }
            }
        }
    }
    __syncthreads();
    // the flush: every cell that is not 0, once, to its place in the caller's tables
    const uint32_t cs = 16u * in.ch;
    if (want_base) for (uint32_t i = threadIdx.x; i < cs * 5u; i += 256u) {
        const unsigned long long v = t_base[i];
        if (!v) continue;
        const uint64_t at = ((uint64_t)mate * in.cycles + pf_slot_cycle(i / 5u, in.ch)) * 5u + i % 5u;
        if (in.base_cnt) atomicAdd(&in.base_cnt[at], v >> 32);
        if (in.base_qsum && (uint32_t)v) atomicAdd(&in.base_qsum[at], v & 0xFFFFFFFFull);
    }
    if (want_qh) for (uint32_t i = threadIdx.x; i < cs * in.qs; i += 256u) {
        const uint32_t v = t_qh[i];
        if (v) atomicAdd(&in.qual_hist[((uint64_t)mate * in.cycles + pf_slot_cycle(i / in.qs, in.ch)) * in.qbins + i % in.qs], (unsigned long long)v);
    }
    if (in.len_hist) for (uint32_t i = threadIdx.x; i < in.len_bins; i += 256u) { const uint32_t v = t_len[i]; if (v) atomicAdd(&in.len_hist[(uint64_t)mate * in.len_bins + i], (unsigned long long)v); }
    if (in.meanq_hist) for (uint32_t i = threadIdx.x; i < in.qbins; i += 256u) { const uint32_t v = t_mq[i]; if (v) atomicAdd(&in.meanq_hist[(uint64_t)mate * in.qbins + i], (unsigned long long)v); }
    if (in.gc_hist) for (uint32_t i = threadIdx.x; i < PF_GC_BINS; i += 256u) { const uint32_t v = t_gc[i]; if (v) atomicAdd(&in.gc_hist[(uint64_t)mate * PF_GC_BINS + i], (unsigned long long)v); }
    pf_sums_out<4>(acc, mate, st);
}

// ---- any row length, any table size
// grid n_rows x 64 threads: a wave per row, everything about the row is the same in every lane.  Tiles lie on the multiples of `tile` from the row's start, so every
// load is a 16-byte group of the row as in the common path.  A position adds to the tables in global memory itself: the path of rows beyond 1024 bytes, of tables
// beyond the LDS, and of the tests.
__global__ void __launch_bounds__(64) k_profile_rows_long(ProfileIn in, ProfileStat* __restrict__ st) {
    const uint64_t g = blockIdx.x; const uint32_t x0 = 16u * threadIdx.x, T = in.tile, mate = in.pairs ? (uint32_t)(g & 1u) : 0u;
    const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u);
    const PfRow r = pf_window(in, g, l, st, threadIdx.x == 0u);
    const uint32_t a = r.a, e = r.a + r.n;
    const uint64_t rowbase = g * in.row_len, crow = (uint64_t)mate * in.cycles;
    const bool mine = x0 < T;                                                // (this lane holds positions of a tile)
    PfAcc acc = {};
    unsigned long long rq = 0ull, rn = 0ull;                                 // the row's score sum; acgt | gc << 32
    if (r.counted && r.n) for (uint32_t t0 = a / T * T; t0 < e; t0 += T) {
        const uint32_t p0 = t0 + x0;
        const uint32_t win = mine ? rows_span(p0, a, e) : 0u;
        if (!win) continue;
        uint32_t b[4] = { 0u, 0u, 0u, 0u }, q[4] = { 0u, 0u, 0u, 0u }, cls[4];
        if (in.b) rows_ld16(in.b, in.vec_in, in.total, rowbase, p0, e, b);
        if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, p0, e, q);
        pf_cut_front(q, p0, a);
        pf_classes(in.ascii, b, cls);
        const unsigned long long t = pf_lane_sums(in, cls, q, win, acc);
        rq += t & 0xFFFFFull; rn += ((t >> 20) & 0xFFFull) | ((t >> 32) << 32);
        if (in.base_cnt || in.base_qsum || in.qual_hist)
            for (uint32_t j = 0; j < 16u; j++) {
                if (!((win >> j) & 1u)) continue;
                uint32_t c = p0 + j - a;
                c = c < in.cycles - 1u ? c : in.cycles - 1u;
                const uint32_t kc = (cls[j >> 2] >> (8u * (j & 3u))) & 7u, qq = (q[j >> 2] >> (8u * (j & 3u))) & 0xFFu;
                const uint64_t at = (crow + c) * 5u + (kc < 4u ? kc : 4u);
                if (in.base_cnt) atomicAdd(&in.base_cnt[at], 1ull);
                if (in.base_qsum && qq) atomicAdd(&in.base_qsum[at], (unsigned long long)qq);
                if (in.qual_hist) atomicAdd(&in.qual_hist[(crow + c) * in.qbins + (qq < in.qbins - 1u ? qq : in.qbins - 1u)], 1ull);
            }
    }
    const unsigned long long qs = wave_sum<unsigned long long>(rq), ng = wave_sum<unsigned long long>(rn);
    if (threadIdx.x == 0u && r.counted) {
        acc.counted = 1ull; acc.max_len = r.n;
        if (in.len_hist) atomicAdd(&in.len_hist[(uint64_t)mate * in.len_bins + pf_len_bin(in, r.n)], 1ull);
        const uint32_t mb = pf_mq_bin(in, r.n, qs), gb = pf_gc_bin(ng & 0xFFFFFFFFull, ng >> 32);
        if (in.meanq_hist && mb != 0xFFFFFFFFu) atomicAdd(&in.meanq_hist[(uint64_t)mate * in.qbins + mb], 1ull);
        if (in.gc_hist && gb != 0xFFFFFFFFu) atomicAdd(&in.gc_hist[(uint64_t)mate * PF_GC_BINS + (gb < PF_GC_BINS ? gb : PF_GC_BINS - 1u)], 1ull);
    }
    pf_sums_out<1>(acc, mate, st);
}
