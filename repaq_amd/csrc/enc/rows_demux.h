// enc/rows_demux.h - rows against one or two sets of barcodes -> a sample per unit, the reason where there is none, the best barcode and its distance per row, the
// keep byte and the start rfq_select_rows takes, a count per sample and one summary (rfq_demux_rows): the step that asks WHOSE a read is, in front of the ones that
// trim, judge, deduplicate and screen.  It decides and moves no bytes.
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose 16-byte loads, unit walk, candidate test, length check and sums it uses, behind
// rows_adapter.h whose base class ar_cls is the rule's, and behind rows_kmer_lanes.h whose sc_lane turns 16 bytes into 2-bit classes and whose sc_win takes the
// window out of them; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the base bytes (include/rfq_hip.h has the rules).  A barcode of up to 32 bases is 2 bits a base, base j in bits 2j and 2j + 1:
// one 32-bit word up to 16 bases, two beyond (the host packs them).  The distance of a window to a barcode is the number of positions that do not agree - the
// classes differ, or the window's byte is of no class 0 .. 3.
//   k_demux_rows<W>            W words a barcode.  256 threads, a LANE per unit, in.steps steps a workgroup.  The sets (and, where it fits, the table of counts per
//                              sample) live in dynamic LDS (at most 34 + 32 KiB: DM_N_MAX, DM_LDS_COUNTS).  A lane loads the one to three 16-byte groups that hold its row's window, turns them into classes and
//                              valid bits (sc_lane), takes the window out of the 96 bits by a funnel shift (sc_win), turns it base 0 lowest once, and walks the set:
//                              every lane reads the SAME LDS word (a broadcast, no bank conflict), x ^ b, the two bits of a position folded into one, the invalid
//                              positions ORed in, a popcount.  d1, best and d2 stay in registers.  The counts are LDS atomics, flushed once per workgroup: one 64-bit
//                              global atomicAdd per cell that is not 0 (rows_profile.h's pattern); beyond DM_LDS_COUNTS cells every unit adds to device memory itself.
//   k_demux_rows_general       RFQ_DEMUX=general, the other formulation: a lane per unit compares byte by byte (ar_cls) against the barcodes' ASCII bytes in device
//                              memory, with plain branches, and counts with global atomics.  The same bytes in every output.
// Both end in dm_unit_out, which is the rule of a unit.  All sums are integers and leave a workgroup as atomic adds: the same bits from run to run.
// No LDS index out of range, by construction: a barcode index is below n[i], a count cell is a sample below n_samples or n_samples itself (a sample comes from best1 *
// n2 + best2 < n1 * n2 = n_samples or from the host's table, whose entries are -1 or below n_samples), and the host launches with the words of exactly these tables.
#define DM_NSUM 9                     // n_candidates, n_assigned, n_exact, why_none, why_ambig, why_short, why_combo, bases_in, bases_out
#define DM_NONE 1u                    // RFQ_DEMUX_* of include/rfq_hip.h
#define DM_AMBIG 2u
#define DM_SHORT 4u
#define DM_COMBO 8u
#define DM_MASKED 128u
#define DM_LEN_MAX 32u
#define DM_N_MAX 4096u                // barcodes of a set at most.  With n1 * n2 <= 2^20 the two sets take at most (4096 + 256) x 2 words = 34 KiB of LDS, the counts 32 KiB more
#define DM_LDS_COUNTS 8192u           // cells (n_samples + 1) the LDS table of counts holds at most: 32 KiB
#ifndef DM_WG_PER_CU
#define DM_WG_PER_CU 4u               // workgroups per compute unit the grid is capped at: a workgroup pays for its copy of the sets and its flush once (-DDM_WG_PER_CU=2u / 8u build the grids DESIGN.md compares it with)
#endif
#define DM_LDS_WORDS (2u * DM_N_MAX * 2u + DM_LDS_COUNTS)
struct DemuxIn {
    const uint8_t* b; const int32_t* lens; const uint8_t* cand;               // cand null: every unit is a candidate
    uint64_t total;                                                           // bytes of the row buffer: n_rows * row_len
    uint32_t n_rows, n_units, row_len;
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffer 16-byte aligned: a lane's group may be loaded whole
    uint32_t ascii, pairs;
    uint32_t n[2], len[2], off[2], skip[2];                                   // set i is read from row i of the unit; n[1] == 0: no set 2
    uint32_t max_mm, min_delta, n_samples;
    uint32_t steps;                                                           // k_demux_rows: steps of a workgroup
    uint32_t lds_counts;                                                      // k_demux_rows: the counts go through LDS
    const uint32_t* packed[2];                                                // [n][W] words, base j in bits 2j, 2j + 1 (8-byte aligned)
    const uint8_t* text[2];                                                   // [n][len] ASCII bytes (k_demux_rows_general)
    const int32_t* table;                                                     // [n1][n2] the sample of a pair of barcodes, -1: not listed; null: best1 * n2 + best2
    int32_t* sample; uint8_t* why; int32_t* best; uint8_t* dist; uint8_t* keep; int32_t* start;       // [U], [U], [n_rows] x 4, or null
    unsigned long long* counts;                                               // [n_samples + 1], zeroed per call, or null
};
typedef RowsSums<DM_NSUM> DemuxStat;
// what a row's walk over its set leaves: the lowest index at the least distance and that distance (-1 / 255: nothing was compared), the row's RFQ_DEMUX_* bits
struct DmRow { int32_t best; uint32_t d1, why; };
__device__ __forceinline__ DmRow dm_no_row(uint32_t why) { DmRow r; r.best = -1; r.d1 = 255u; r.why = why; return r; }
__device__ __forceinline__ DmRow dm_verdict(const DemuxIn& in, uint32_t best, uint32_t d1, uint32_t d2) {
    DmRow r; r.best = (int32_t)best; r.d1 = d1;
    r.why = d1 > in.max_mm ? DM_NONE : (d2 - d1 < in.min_delta ? DM_AMBIG : 0u);
    return r;
}

// ---- a unit's verdict
// The unit's lane writes its outputs and adds it to the sums it keeps for the workgroup (l: its rows' lengths; r: its rows' walks, dm_no_row(0) for a row without a
// set and for every row of a unit that is no candidate).  Returns the cell of d_counts the unit belongs to, ~0 for a unit that is no candidate.
__device__ __forceinline__ uint32_t dm_unit_out(const DemuxIn& in, uint64_t u, bool cand, const uint32_t (&l)[2], const DmRow (&r)[2], unsigned long long (&acc)[DM_NSUM]) {
    const uint32_t nr = in.pairs ? 2u : 1u;
    uint32_t why = cand ? (r[0].why | r[1].why) : DM_MASKED;
    int32_t sample = -1;
    if (cand && why == 0u) {
        if (!in.n[1]) sample = r[0].best;
        else {
            const uint32_t at = (uint32_t)r[0].best * in.n[1] + (uint32_t)r[1].best;
            sample = in.table ? in.table[at] : (int32_t)at;
            if (sample < 0 || (uint32_t)sample >= in.n_samples) { sample = -1; why = DM_COMBO; }
        }
    }
    const bool assigned = cand && why == 0u;
    if (in.sample) in.sample[u] = sample;
    if (in.why) in.why[u] = (uint8_t)why;
    unsigned long long lsum = 0ull, osum = 0ull;
#pragma unroll
    for (uint32_t i = 0; i < 2u; i++) {                                      // (a constant bound: l and r stay in registers)
        if (i >= nr) break;
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        const bool has_set = i == 0u || in.n[1] != 0u;
        const uint32_t cut = in.off[i] + in.len[i] + in.skip[i], st = assigned && has_set ? (cut < l[i] ? cut : l[i]) : 0u;
        if (in.best) in.best[g] = r[i].best;
        if (in.dist) in.dist[g] = (uint8_t)r[i].d1;
        if (in.keep) in.keep[g] = assigned ? 1u : 0u;
        if (in.start) in.start[g] = (int32_t)st;
        lsum += l[i]; osum += l[i] - st;
    }
    if (!cand) return 0xFFFFFFFFu;
    acc[0] += 1ull; acc[1] += assigned; acc[2] += assigned && r[0].d1 == 0u && (!in.n[1] || r[1].d1 == 0u);
    acc[3] += (why & DM_NONE) != 0u; acc[4] += (why & DM_AMBIG) != 0u; acc[5] += (why & DM_SHORT) != 0u; acc[6] += (why & DM_COMBO) != 0u;
    acc[7] += lsum; acc[8] += assigned ? osum : 0ull;
    return assigned ? (uint32_t)sample : in.n_samples;
}

// ---- a row's window as 2-bit classes
// x: base j of the window in bits 2j, 2j + 1; inv: bit 2j set where position j is of no class 0 .. 3.  Both are 0 beyond the window's len positions.
struct DmWin { unsigned long long x, inv; };
// the 2n bits of x (right-aligned, the first base highest) with the first base lowest
__device__ __forceinline__ unsigned long long dm_turn(unsigned long long x, uint32_t n) {
    const unsigned long long r = (((unsigned long long)sc_brev32((uint32_t)x) << 32) | sc_brev32((uint32_t)(x >> 32))) >> (64u - 2u * n);
    return ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
}
// Row g of l bases, l >= off + len: the one to three 16-byte groups that hold [off, off + len) - only bytes in front of l, so never outside the rows.
__device__ __forceinline__ DmWin dm_window(const DemuxIn& in, uint64_t g, uint32_t l, uint32_t off, uint32_t len) {
    const uint32_t g0 = off & ~15u, sh = off & 15u, ng = (sh + len + 15u) >> 4;
    uint32_t w[3] = { 0u, 0u, 0u }, v[3] = { 0u, 0u, 0u };
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        if (k >= ng) continue;
        uint32_t b[4];
        rows_ld16(in.b, in.vec_in, in.total, g * in.row_len, g0 + 16u * k, l, b);
        const ScLane a = sc_lane(in.ascii, b, rows_span(g0 + 16u * k, 0u, l));
        w[k] = a.w; v[k] = a.v;
    }
    const unsigned long long V = (unsigned long long)v[0] | ((unsigned long long)v[1] << 16) | ((unsigned long long)v[2] << 32);
    const uint32_t bad = ~(uint32_t)(V >> sh) & (len >= 32u ? 0xFFFFFFFFu : (1u << len) - 1u);
    DmWin r;
    r.x = dm_turn(sc_win(w[0], w[1], w[2], 2u * sh, len), len);
    r.inv = (unsigned long long)sc_spread16(bad & 0xFFFFu) | ((unsigned long long)sc_spread16(bad >> 16) << 32);
    return r;
}
// The walk over a set of n barcodes of W words each (LDS: every lane reads the same word).  Called by lanes that have a window.
template <int W> __device__ __forceinline__ DmRow dm_walk(const DemuxIn& in, const uint32_t* set, uint32_t n, uint32_t len, const DmWin& win) {
    uint32_t d1 = len + 1u, d2 = len + 1u, best = 0u;
    if constexpr (W == 1) {
        const uint32_t x = (uint32_t)win.x, inv = (uint32_t)win.inv;
#pragma unroll 4
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t t = x ^ set[i], d = (uint32_t)__popc(((t | (t >> 1)) & 0x55555555u) | inv);
            if (d < d1) { d2 = d1; d1 = d; best = i; } else if (d < d2) d2 = d;
        }
    } else {
        const unsigned long long* const s64 = (const unsigned long long*)set;
#pragma unroll 4
        for (uint32_t i = 0; i < n; i++) {
            const unsigned long long t = win.x ^ s64[i]; const uint32_t d = (uint32_t)__popcll(((t | (t >> 1)) & 0x5555555555555555ull) | win.inv);
            if (d < d1) { d2 = d1; d1 = d; best = i; } else if (d < d2) d2 = d;
        }
    }
    return dm_verdict(in, best, d1, d2);
}

// grid ceil(n_units / (256 * steps)) x 256 threads; dynamic LDS: (n1 + n2) * W words of the sets, then n_samples + 1 words of counts with in.lds_counts.  A lane
// takes a unit per step (UnitGroup<1>).  ALL rows' lengths are checked, candidates or not; only a candidate's bytes are loaded.
template <int W> __global__ void __launch_bounds__(256) k_demux_rows(DemuxIn in, DemuxStat* __restrict__ st) {
    // (declared in 64-bit words: a two-word barcode is read as one.  The interpreter's buffer for dynamic LDS holds 64 KB; there the tables get a block of their own,
    // of the size the host never exceeds)
#ifdef RFQ_SIMT_EMULATION
    __shared__ unsigned long long dm_lds64[DM_LDS_WORDS / 2u];
#else
    RFQ_DYN_SHARED(unsigned long long, dm_lds64);
#endif
    uint32_t* const dm_lds = (uint32_t*)dm_lds64;
    const uint32_t w0 = in.n[0] * (uint32_t)W, w1 = in.n[1] * (uint32_t)W, cells = in.n_samples + 1u;
    uint32_t* const set0 = dm_lds; uint32_t* const set1 = dm_lds + w0; uint32_t* const cnt = dm_lds + w0 + w1;
    for (uint32_t i = threadIdx.x; i < w0; i += 256u) set0[i] = in.packed[0][i];
    for (uint32_t i = threadIdx.x; i < w1; i += 256u) set1[i] = in.packed[1][i];
    if (in.lds_counts) for (uint32_t i = threadIdx.x; i < cells; i += 256u) cnt[i] = 0u;
    __syncthreads();
    const UnitGroup<1> ug{};
    const uint32_t nr = in.pairs ? 2u : 1u;
    unsigned long long acc[DM_NSUM] = {};
    for (uint32_t it = 0; it < in.steps; it++) {
        const uint64_t u = ug.unit(it, in.steps);
        if (ug.past(u, in.n_units)) break;
        if (u >= in.n_units) continue;
        const bool cand = rows_cand(in, u);
        uint32_t l[2] = { 0u, 0u }; DmRow r[2] = { dm_no_row(0u), dm_no_row(0u) };
#pragma unroll
        for (uint32_t i = 0; i < 2u; i++) {                                  // (a constant bound: l and r stay in registers)
            if (i >= nr) break;
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            l[i] = rows_len_checked(in, g, st, true);
            if (!cand || !in.n[i]) continue;
            if (l[i] < in.off[i] + in.len[i]) { r[i] = dm_no_row(DM_SHORT); continue; }
            r[i] = dm_walk<W>(in, i ? set1 : set0, in.n[i], in.len[i], dm_window(in, g, l[i], in.off[i], in.len[i]));
        }
        const uint32_t cell = dm_unit_out(in, u, cand, l, r, acc);
        if (in.counts && cell != 0xFFFFFFFFu) { if (in.lds_counts) atomicAdd(&cnt[cell], 1u); else atomicAdd(&in.counts[cell], 1ull); }
    }
    __syncthreads();
    // the flush: every cell that is not 0, once (a workgroup sees fewer than 2^31 units: no cell wraps)
    if (in.counts && in.lds_counts) for (uint32_t i = threadIdx.x; i < cells; i += 256u) { const uint32_t v = cnt[i]; if (v) atomicAdd(&in.counts[i], (unsigned long long)v); }
    rows_sums_out<4>(acc, st->c);
}

// ---- the other formulation
// grid ceil(n_units / 256) x 256 threads, a lane per unit: every position of the window against every barcode's byte, one by one - only bytes in front of a read's
// length, so never outside the rows.
__device__ __forceinline__ DmRow dm_walk_bytes(const DemuxIn& in, const uint8_t* row, uint32_t i) {
    const uint32_t n = in.n[i], len = in.len[i]; const uint8_t* const x = row + in.off[i];
    uint32_t d1 = len + 1u, d2 = len + 1u, best = 0u;
    for (uint32_t k = 0; k < n; k++) {
        const uint8_t* const bc = in.text[i] + (size_t)k * len;
        uint32_t d = 0u;
        for (uint32_t j = 0; j < len; j++) {
            const uint32_t c = ar_cls(in.ascii, x[j]);
            if (c > 3u || c != ar_cls(1u, bc[j])) d++;
        }
        if (d < d1) { d2 = d1; d1 = d; best = k; } else if (d < d2) d2 = d;
    }
    return dm_verdict(in, best, d1, d2);
}
__global__ void __launch_bounds__(256) k_demux_rows_general(DemuxIn in, DemuxStat* __restrict__ st) {
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t nr = in.pairs ? 2u : 1u;
    unsigned long long acc[DM_NSUM] = {};
    if (u < in.n_units) {
        const bool cand = rows_cand(in, u);
        uint32_t l[2] = { 0u, 0u }; DmRow r[2] = { dm_no_row(0u), dm_no_row(0u) };
#pragma unroll
        for (uint32_t i = 0; i < 2u; i++) {                                  // (a constant bound: l and r stay in registers)
            if (i >= nr) break;
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            l[i] = rows_len_checked(in, g, st, true);
            if (!cand || !in.n[i]) continue;
            if (l[i] < in.off[i] + in.len[i]) { r[i] = dm_no_row(DM_SHORT); continue; }
            r[i] = dm_walk_bytes(in, in.b + g * in.row_len, i);
        }
        const uint32_t cell = dm_unit_out(in, u, cand, l, r, acc);
        if (in.counts && cell != 0xFFFFFFFFu) atomicAdd(&in.counts[cell], 1ull);
    }
    rows_sums_out<4>(acc, st->c);
}
