// enc/rows_group.h - rows -> the kept rows GROUPED by an integer bin per unit, trimmed to a window each, with their lengths, names, name offsets and the first
// output row of every bin (rfq_group_rows): a stable partition of the units by bin, in ONE pass over the rows - what one rfq_select_rows call per bin gives, bin
// after bin.  Part of rfq_encode_kernels.h (included from there, behind enc/rows_select.h; not a stand-alone header).
#pragma once
// k_group_judge is rfq_select_rows' judging pass (sel_judge, enc/rows_select.h) under one more rule: a unit - a row, with pairs the rows 2k / 2k + 1 - has a bin;
// bin < 0 goes to the rest bin or falls, bin >= n_bins refuses the call.  It leaves ONE word per unit (the bin as a key of at most 16 bits, all ones for a unit
// that falls), the sums a size query answers - rows and name bytes kept among them: nothing is scanned in input order - and a bit per bin that holds a row.
// After ONE read-back the host decides.  The order is made by a stable LSD radix sort of (key, unit) over the kept units in 8-bit digits: ONE pass up to 256 bins,
// two beyond.  A pass is k_gr_hist (a digit histogram per tile of GR_TILE elements into a digit-major table [256][tiles]), the host's scan_exclusive over that table
// and k_gr_scatter; the first pass reads the judge's words and so compacts as it sorts.  k_group_tables then makes, a thread per OUTPUT unit, the table entry
// (SelRow), the length and the name size of its rows; the name sizes are scanned in OUTPUT order, and rfq_select_rows' two writers (k_sel_rows, k_sel_names) follow
// the tables as they are.  k_group_bin_off finds every bin's first unit in the sorted keys.  No atomic decides where a row goes: the same bytes from run to run.
#define GR_ERR_BIN     (1u << 3)      // a bin >= n_bins (beside SL_ERR_*; RFQ_E_ARG)
#define GR_MAX_BINS    65536u         // bins of a call, the rest bin included: a key has 16 bits
#define GR_DROPPED     0xFFFFFFFFu    // the judge's word of a unit that falls
#define GR_STEPS       8u
#define GR_TILE        (256u * GR_STEPS)      // elements of a workgroup of the sort: 2048
// what the host reads back: SelStat's fields where sel_judge and rows_sizes_reduce look for them, then the rule's own; zeroed per call, bad_row = bad_unit = ~0
struct GroupStat { uint32_t err, max_len, max_name, n_used; unsigned long long bad_row, n_bases, d_mask, d_short, d_mate, d_bin, n_kept, names_len, bad_unit; };
struct GroupIn {
    const int32_t* bin;                       // [units]
    uint32_t* kk;                             // [units] out: the unit's key, GR_DROPPED where it falls
    uint32_t* used;                           // [words] a bit per bin that holds a row, zeroed by the host
    uint32_t n_bins, rest, words;             // (words: ceil((n_bins + rest) / 32))
};

// The rule of rfq_group_rows as sel_judge takes it.  Both rows of a pair reach the same verdict (each looks at its mate), so the even row's thread writes the unit's
// word.  The bins that hold a row are collected in an LDS bitmap per workgroup and flushed once: a word goes to device memory only where it adds a bit.
struct GroupRule {
    const GroupIn& gi; uint32_t pairs; uint32_t* s_used;
    uint32_t key = 0, nk = 0; unsigned long long ns = 0;
    __device__ __forceinline__ bool drops(uint32_t g, uint32_t& err) {
        const int32_t b = gi.bin[g >> pairs];
        key = 0;
        if (b >= 0 && (uint32_t)b >= gi.n_bins) { err = GR_ERR_BIN; return false; }
        if (b < 0) { key = gi.n_bins; return gi.rest == 0; }
        key = (uint32_t)b;
        return false;
    }
    __device__ __forceinline__ void bad(GroupStat* st, uint32_t g) const { atomicMin(&st->bad_unit, (unsigned long long)(g >> pairs)); }
    __device__ __forceinline__ void row(uint32_t g, bool kept, uint64_t nl) {
        if (!(g & pairs)) gi.kk[g >> pairs] = kept ? key : GR_DROPPED;
        if (kept) { nk++; ns += nl; atomicOr(&s_used[key >> 5], 1u << (key & 31u)); }
    }
    __device__ __forceinline__ void finish(GroupStat* st, uint32_t dr) {
        const uint32_t a = wave_sum(dr), b = wave_sum(nk); const unsigned long long c = wave_sum<unsigned long long>(ns);
        if (lane_id() == 0) {
            if (a) atomicAdd(&st->d_bin, (unsigned long long)a);
            if (b) atomicAdd(&st->n_kept, (unsigned long long)b);
            if (c) atomicAdd(&st->names_len, c);
        }
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < gi.words; w += 256u) {
            const uint32_t v = s_used[w];
            if (v && (__atomic_load_n(gi.used + w, __ATOMIC_RELAXED) & v) != v) atomicOr(gi.used + w, v);
        }
    }
};
// grid ceil(n_rows / SJ_ROWS) x 256 threads: sel_judge's
__global__ void __launch_bounds__(256) k_group_judge(SelIn in, GroupIn gi, GroupStat* __restrict__ st) {
    __shared__ uint32_t s_used[GR_MAX_BINS / 32u];
    for (uint32_t w = threadIdx.x; w < gi.words; w += 256u) s_used[w] = 0;
    __syncthreads();
    GroupRule rule{ gi, in.pairs, s_used };
    sel_judge(in, st, rule);
}
// one workgroup of 256 threads: the bins that hold a row, counted
__global__ void __launch_bounds__(256) k_group_used(const uint32_t* __restrict__ used, uint32_t words, GroupStat* __restrict__ st) {
    uint32_t c = 0;
    for (uint32_t w = threadIdx.x; w < words; w += 256u) c += (uint32_t)__popcll((unsigned long long)used[w]);
    c = wave_sum(c);
    if (lane_id() == 0 && c) atomicAdd(&st->n_used, c);
}

// ---- the stable rank: one pass of the radix sort.  The elements of a pass: the judge's words (key null) - element i is unit i, there where kk[i] is a key -, or a
// sorted pair of arrays, all of them.  The digit of an element is (key >> shift) & 255.
struct GrSrc { const uint32_t* kk; const uint16_t* key; const uint32_t* idx; uint32_t n, shift; };
__device__ __forceinline__ bool gr_load(const GrSrc& s, uint64_t i, uint32_t& key, uint32_t& idx) {
    key = 0; idx = 0;
    if (i >= s.n) return false;
    if (s.key) { key = s.key[i]; idx = s.idx[i]; return true; }
    key = s.kk[i]; idx = (uint32_t)i;
    return key != GR_DROPPED;
}
// The lanes of the wave that hold an element with this lane's digit (none for a lane without one): eight ballots, one per bit of the digit.  All 64 lanes call it.
__device__ __forceinline__ unsigned long long gr_peers(uint32_t digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const uint32_t bit = (digit >> b) & 1u;
        const unsigned long long v = __ballot(valid && bit);
        m &= bit ? v : ~v;
    }
    return valid ? m : 0ull;
}
// grid tiles x 256 threads.  A wave takes 64 consecutive elements per step; the lowest lane of every set of peers adds their number to the tile's LDS histogram
// (counts only: their order does not matter).  hist[d * tiles + tile] = elements of the tile with digit d.
__global__ void __launch_bounds__(256) k_gr_hist(GrSrc s, uint32_t tiles, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * GR_TILE + threadIdx.x;
    const unsigned long long below = (1ull << lane_id()) - 1ull;
#pragma unroll
    for (uint32_t st = 0; st < GR_STEPS; st++) {
        uint32_t key, idx; const bool valid = gr_load(s, t0 + st * 256u, key, idx);
        const uint32_t d = (key >> s.shift) & 255u;
        const unsigned long long peers = gr_peers(d, valid);
        if (valid && !(peers & below)) atomicAdd(&s_h[d], (uint32_t)__popcll(peers));
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * tiles + blockIdx.x] = s_h[threadIdx.x];
}
// grid tiles x 256 threads; base[] is hist[] scanned: the first output position of the tile's elements with digit d.  The rank of an element inside its tile is
// stable by construction: rank in the wave = the peers below the lane; the wave's count per digit goes to the LDS table s_c[step x wave][256], whose rows are in
// input order (step, wave, lane); thread d prefixes column d.  Position = base + the prefix of the element's row + its rank in the wave.
__global__ void __launch_bounds__(256) k_gr_scatter(GrSrc s, uint32_t tiles, const uint32_t* __restrict__ base, uint16_t* __restrict__ okey, uint32_t* __restrict__ oidx) {
    __shared__ uint16_t s_c[GR_STEPS * 4u][256];
    __shared__ uint32_t s_base[256];
#pragma unroll
    for (uint32_t r = 0; r < GR_STEPS * 4u; r++) s_c[r][threadIdx.x] = 0;
    s_base[threadIdx.x] = base[(uint64_t)threadIdx.x * tiles + blockIdx.x];
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * GR_TILE + threadIdx.x;
    const unsigned long long below = (1ull << lane_id()) - 1ull;
    const uint32_t wv = (uint32_t)wave_id();
    uint32_t key[GR_STEPS], idx[GR_STEPS], dr[GR_STEPS];                     // dr: digit | rank in the wave << 8 | 1 << 31; 0 = no element
#pragma unroll
    for (uint32_t st = 0; st < GR_STEPS; st++) {
        const bool valid = gr_load(s, t0 + st * 256u, key[st], idx[st]);
        const uint32_t d = (key[st] >> s.shift) & 255u;
        const unsigned long long peers = gr_peers(d, valid);
        const unsigned long long lower = peers & below;
        if (valid && !lower) s_c[st * 4u + wv][d] = (uint16_t)__popcll(peers);
        dr[st] = valid ? (d | ((uint32_t)__popcll(lower) << 8) | 0x80000000u) : 0u;
    }
    __syncthreads();
    {
        uint32_t run = 0;
#pragma unroll
        for (uint32_t r = 0; r < GR_STEPS * 4u; r++) { const uint32_t t = s_c[r][threadIdx.x]; s_c[r][threadIdx.x] = (uint16_t)run; run += t; }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t st = 0; st < GR_STEPS; st++) {
        if (!(dr[st] >> 31)) continue;
        const uint32_t d = dr[st] & 255u, pos = s_base[d] + s_c[st * 4u + wv][d] + ((dr[st] >> 8) & 63u);
        okey[pos] = (uint16_t)key[st]; oidx[pos] = idx[st];
    }
}

// ---- tables, in OUTPUT order.  grid ceil(n_units / 256) x 256 threads, a thread per output unit j = input unit sidx[j]: the SelRow of its row (with pairs: of both),
// the caller's lens and the bytes of the row's name (64-bit: scanned by the host to the output offsets; null for rows without names).
__global__ void __launch_bounds__(256) k_group_tables(SelIn in, const uint32_t* __restrict__ sidx, uint32_t n_units, SelRow* __restrict__ tab, uint64_t* __restrict__ nsz,
                                                      int32_t* __restrict__ d_lens) {
    const uint64_t j64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j64 >= n_units) return;
    const uint32_t nr = in.pairs ? 2u : 1u, u = sidx[j64];
    for (uint32_t r = 0; r < nr; r++) {
        const uint32_t row = u * nr + r, o = (uint32_t)j64 * nr + r;
        uint32_t s0, w, e; (void)sel_window(in, row, s0, w, e);
        *(uint4*)(tab + o) = make_uint4(row, s0, w, 0u);
        if (d_lens) d_lens[o] = (int32_t)w;
        if (nsz) nsz[o] = in.name_off[row + 1] - in.name_off[row];
    }
}
// grid ceil((T + 1) / 256) x 256 threads: bin_off[b] = the first output ROW of bin b - the first sorted key >= b, times the rows of a unit; empty bins included
__global__ void __launch_bounds__(256) k_group_bin_off(const uint16_t* __restrict__ skey, uint32_t n_units, uint32_t T, uint32_t nr, uint64_t* __restrict__ bin_off) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b > T) return;
    uint32_t lo = 0, hi = n_units;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (skey[mid] < b) lo = mid + 1u; else hi = mid; }
    bin_off[b] = (uint64_t)lo * nr;
}
