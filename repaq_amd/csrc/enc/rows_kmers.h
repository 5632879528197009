// enc/rows_kmers.h - rows -> a table of the canonical k-mers they hold with a count beside each value, in a caller-owned buffer that adds up across calls
// (rfq_kmers_init, rfq_kmers_rows), and such a table -> its spectrum, its (value, count) list and a screen index of the selected values (rfq_kmers_read): the k-mer
// section of a QC report, the k-mer spectrum, screening by abundance.
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h and behind rows_kmer_lanes.h whose k-mers of a row - sc_kmers_row, sc_kmers_row_long - and
// set - the slot format, the screen index's header, sc_start, sc_claim - it uses as they stand; not a stand-alone header).
#pragma once
// The k-mer rules are rfq_screen_rows' (include/rfq_hip.h).  The table is a 64-byte header, S slots of 64 bits (0 = empty, else bit 63 | canonical value: the
// screen index's slot and linear probing, its hash sc_start applied to the value mixed - km_start) and S counts of 64 bits, count[s] beside slot[s].  A slot is
// claimed with sc_claim, and count[s] is added to only once slot[s] is known to hold the value; no kernel reads a count it adds to.
//   k_kmers_rows<16> / <64>    the screen's common path (a row of up to 256 / 1024 bytes held by 16 lanes / by a wave, a lane's 16 positions from three words).
//                              LDS = true: the workgroup first combines in a table of KM_LDS_SLOTS (value, count) pairs in LDS - claimed with an LDS compare-and-
//                              swap, added to with LDS atomics; a k-mer that finds no LDS slot within KM_LDS_PROBES probes goes straight to device memory - and
//                              flushes every LDS entry at its end with ONE claim and ONE 64-bit atomicAdd of the entry's count: 290 M adds onto 512 values (k = 5)
//                              leave the compute unit as a few hundred thousand.  LDS = false (RFQ_KMERS=direct): every k-mer goes to device memory.
//   k_kmers_rows_long          any row length (and every call with RFQ_KMERS=general): a wave per row, tiles of 1024 bases, adds straight to device memory.
//   k_kmers_hdr                one thread: the call's sums into the header (n_kmers, total, the INCOMPLETE flag when a k-mer was lost).
//   k_kmers_count              a lane per slot: entries, sum of counts, the selected ones and their sum, the largest count.
//   k_kmers_write              a lane per slot: the spectrum (bins in LDS where hist_len fits, flushed once), the list (a cursor reserved once per wave) and
//                              the screen index of the selected values (k_screen_build's claim: entries are re-inserted, never copied slot by slot).
// A probe walk takes at most min(S, KM_WALK) steps (S under the collide flag), every slot number is masked to S: a table that was written over cannot hang a call or
// take it outside its S slots and S counts.  A k-mer whose walk ends without an empty slot or its own value is LOST and counted as such: the host refuses the call.
// All sums are integers and leave a workgroup through rows_sums_out.  A count is 64 bits wide and every add to one is a 64-bit atomicAdd (counts past 2^32 are not
// reached by any test: a few-second test cannot add that often); an LDS entry's count is 32 bits, which a workgroup's rows never fill (KM_STEPS_MAX).
#define KM_NSUM 5                     // n_counted, bases_in, added, n_new, lost
#define KM_RSUM 6                     // n_kmers, total, n_selected, selected_total (sums); max_count (an atomicMax); the list's cursor
#define KM_MAGIC 0x31424154524D4B52ull        // "RKMRTAB1"
#define KM_VERSION 1u
#define KM_FLAG_COLLIDE 1u
#define KM_FLAG_INCOMPLETE 2u
#define KM_WALK 512u                  // steps of a probe walk at most (load <= 1/2, the sizing rule: runs of that length do not occur; a table filled beyond it is refused)
#define KM_COLLIDE_SLOTS 65536u       // under the collide flag chains are as long as the table is full: no larger table is formatted
#ifndef KM_LDS_SLOTS
#define KM_LDS_SLOTS 2048u            // (value, count) pairs of a workgroup's LDS table: 24 KiB, six workgroups of 256 threads a compute unit (a power of two; DESIGN.md has the sizes tried: 512 and 8192 are slower)
#endif
#define KM_LDS_PROBES 4u
#define KM_ITER 4u                    // steps of a workgroup at least
#define KM_STEPS_MAX 2048u            // steps of a workgroup at most: 2048 * 16 rows * 1024 positions < 2^32, an LDS count cannot wrap
#define KM_WG_PER_CU 8u               // the common path's grid: workgroups per compute unit - a workgroup pays for its flush once
#define KM_READ_ITER 16u              // slots a lane of the read's kernels takes
#define KM_HIST_LDS 4096u             // bins the read keeps in LDS at most
struct KmersHdr { unsigned long long magic; uint32_t version, k; unsigned long long S, n_kmers, total; uint32_t flags, pad[5]; };
static_assert(sizeof(KmersHdr) == 64, "the table header is 64 bytes");
struct KmersIn {
    const uint8_t* b; const int32_t* lens; const uint8_t* cand;               // cand null: every row is counted
    uint64_t total;                                                           // bytes of the row buffer: n_rows * row_len
    uint32_t n_rows, row_len, vec_in, ascii;
    uint32_t k, collide, walk;                                                // of the table's header; walk: min(S, KM_WALK), S under collide
    uint32_t steps;                                                           // common path: steps of a workgroup
    unsigned long long* tab; unsigned long long* cnt; uint64_t S;             // the slots and the counts (S a power of two)
    uint32_t* kmers;                                                          // [n_rows] or null
};
struct KmersReadIn {
    const unsigned long long* tab; const unsigned long long* cnt; uint64_t S;
    unsigned long long min_count, max_count;                                  // selected: min_count <= count and (max_count == 0 or count <= max_count); min_count >= 1
    unsigned long long* hist; uint32_t hist_len;
    unsigned long long* values; unsigned long long* counts; uint64_t list_cap;
    ScreenHdr* ihdr; unsigned long long* itab; uint64_t iS; uint32_t k, icollide;
};
typedef RowsSums<KM_NSUM> KmersStat;
typedef RowsSums<KM_RSUM> KmersReadStat;

// ---- the add
// c occurrences of the canonical value v into the table in device memory; acc: [2] added, [3] n_new, [4] lost
// The start slot is sc_start of the value MIXED: sc_start alone takes bits 20 and up of v * c, which the last 10 + log2(S) / 2 bases of a k-mer decide - and reads
// are full of k-mers that share those and differ in front of them (every read that runs into a poly-A or poly-G tail, every repeat in another context): they would
// all start at one slot and grow chains past any bound.  One multiplication and one fold more let every base of the k-mer reach every bit of the start slot.  The
// slot holds the value itself; the screen index rfq_kmers_read makes is hashed as rfq_screen_build hashes (its lookup is rfq_screen_rows').
__device__ __forceinline__ unsigned long long km_mul(unsigned long long v) { return v * 0xFF51AFD7ED558CCDull; }
__device__ __forceinline__ uint64_t km_start(unsigned long long v, uint64_t mask, uint32_t collide) { const unsigned long long m = km_mul(v); return sc_start(m ^ (m >> 32), mask, collide); }
__device__ __forceinline__ void km_add_dev(const KmersIn& in, unsigned long long v, unsigned long long c, unsigned long long (&acc)[KM_NSUM]) {
    const uint64_t mask = in.S - 1ull;
    const ScSlot at = sc_claim(in.tab, mask, km_start(v, mask, in.collide), sc_key(v), in.walk);
    const bool held = at.s != SC_NO_SLOT;
    if (held) atomicAdd(&in.cnt[at.s], c);                                   // (64 bits: a hot value's count passes 2^32 in a large file)
    // (every sum under its own constant index, no branch between them: the compiler folds `acc[2] += c` and `acc[4] += c` on two paths into one add at a computed
    // index, and sums indexed like that live in scratch)
    acc[2] += held ? c : 0ull; acc[3] += at.claimed ? 1ull : 0ull; acc[4] += held ? 0ull : c;
}
__device__ __forceinline__ uint32_t km_lds_start(unsigned long long v) { return (uint32_t)(km_mul(v) >> 40) & (KM_LDS_SLOTS - 1u); }       // (bits 40 and up: every base but the first few of k > 25)
// one occurrence: into the workgroup's LDS table where a slot is free or holds the value within KM_LDS_PROBES probes, else into device memory.  (The LDS walk is
// not sc_claim: 32-bit slot numbers, a volatile LDS read where that one takes an agent-scope load, and the count is added inside the walk.)
template <bool LDS> __device__ __forceinline__ void km_add(const KmersIn& in, unsigned long long* lk, uint32_t* lc, unsigned long long v, unsigned long long (&acc)[KM_NSUM]) {
    if constexpr (LDS) {
        const unsigned long long key = sc_key(v);
        uint32_t s = km_lds_start(v);
        for (uint32_t n = 0; n < KM_LDS_PROBES; n++) {
            unsigned long long cur = ((volatile unsigned long long*)lk)[s];
            if (cur == 0ull) { cur = atomicCAS(&lk[s], 0ull, key); if (cur == 0ull) cur = key; }
            if (cur == key) { atomicAdd(&lc[s], 1u); return; }
            s = (s + 1u) & (KM_LDS_SLOTS - 1u);
        }
    }
    km_add_dev(in, v, 1ull, acc);
}
__device__ __forceinline__ bool km_counted(const KmersIn& in, uint64_t g) { return !in.cand || in.cand[g] != 0u; }

// grid ceil(n_rows / (256 / LPR * steps)) x 256 threads.  A group of the workgroup (UnitGroup: LPR lanes) takes a row per step, in.steps steps.  ALL rows' lengths
// are checked, counted or not; only a counted row's bytes are loaded.  What depends on the row only masks: the lane moves (inside sc_kmers_row) and the reductions
// are called by every lane of the wave.  Every valid k-mer is added where it is formed (sc_kmers_row<1>: the add's walks are not copied 16 times).
template <int LPR, bool LDS> __global__ void __launch_bounds__(256) k_kmers_rows(KmersIn in, KmersStat* __restrict__ st) {
    const UnitGroup<LPR> ug{};
    // (a static block on the GPU and under the interpreter, whose buffer for dynamic LDS holds 64 KB)
    __shared__ unsigned long long km_key[LDS ? KM_LDS_SLOTS : 1u];
    __shared__ uint32_t km_cnt[LDS ? KM_LDS_SLOTS : 1u];
    if constexpr (LDS) {
        for (uint32_t i = threadIdx.x; i < KM_LDS_SLOTS; i += 256u) { km_key[i] = 0ull; km_cnt[i] = 0u; }
        __syncthreads();
    }
    unsigned long long acc[KM_NSUM] = {};
    for (uint32_t it = 0; it < in.steps; it++) {
        const uint64_t g = ug.unit(it, in.steps);
        if (ug.past(g, in.n_rows)) break;
        const bool live = g < in.n_rows, counted = live && km_counted(in, g);
        const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u;
        const uint32_t nk = grp_sum<LPR>(sc_kmers_row<1>(in, ug, g, l, counted, [&](unsigned long long v) __attribute__((always_inline)) { km_add<LDS>(in, km_key, km_cnt, v, acc); }));
        if (ug.gl == 0u && live) {
            if (in.kmers) in.kmers[g] = nk;                                  // (0 for a row that is not counted: none of its bytes was loaded)
            if (counted) { acc[0] += 1ull; acc[1] += l; }
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < KM_LDS_SLOTS; i += 256u) {
            const unsigned long long key = km_key[i];
            if (key) km_add_dev(in, key & ~(1ull << 63), (unsigned long long)km_cnt[i], acc);
        }
    }
    rows_sums_out<4>(acc, st->c);
}

// grid n_rows x 64 threads: a wave per row, sc_kmers_row_long's walk; every k-mer goes straight to device memory
__global__ void __launch_bounds__(64) k_kmers_rows_long(KmersIn in, KmersStat* __restrict__ st) {
    const uint64_t g = blockIdx.x;
    const bool counted = km_counted(in, g);
    unsigned long long acc[KM_NSUM] = {};
    const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u);
    const uint32_t nk = sc_kmers_row_long<1>(in, g, l, counted, [&](unsigned long long v) __attribute__((always_inline)) { km_add_dev(in, v, 1ull, acc); });
    const uint32_t t = wave_sum<uint32_t>(nk);
    if (threadIdx.x == 0u) {
        if (in.kmers) in.kmers[g] = t;
        if (counted) { acc[0] += 1ull; acc[1] += l; }
    }
    rows_sums_out<1>(acc, st->c);
}
// 1 x 64 threads, behind the rows kernel on the stream: what the call added goes into the header; a lost k-mer marks the table
__global__ void __launch_bounds__(64) k_kmers_hdr(KmersHdr* hdr, const KmersStat* __restrict__ st) {
    if (threadIdx.x != 0u) return;
    hdr->n_kmers += st->c[3]; hdr->total += st->c[2];
    if (st->c[4]) hdr->flags |= KM_FLAG_INCOMPLETE;
}
// 1 x 64 threads, behind the memset of the whole table: the header of an empty table
__global__ void __launch_bounds__(64) k_kmers_format(KmersHdr* hdr, uint32_t k, unsigned long long S, uint32_t flags) {
    if (threadIdx.x != 0u) return;
    hdr->magic = KM_MAGIC; hdr->version = KM_VERSION; hdr->k = k; hdr->S = S; hdr->flags = flags;
}

// ---- the read.  An ENTRY is a slot that is not empty with a count that is not 0 (a claimed slot's count is added in the kernel that claims it).
__device__ __forceinline__ bool km_selected(const KmersReadIn& in, unsigned long long c) { return c >= in.min_count && (in.max_count == 0ull || c <= in.max_count); }
// grid ceil(S / (256 * KM_READ_ITER)) x 256 threads, a lane per slot and step
__global__ void __launch_bounds__(256) k_kmers_count(KmersReadIn in, KmersReadStat* __restrict__ st) {
    __shared__ unsigned long long s_mx;
    if (threadIdx.x == 0u) s_mx = 0ull;
    __syncthreads();
    unsigned long long acc[4] = {}, mx = 0ull;
    for (uint32_t it = 0; it < KM_READ_ITER; it++) {
        const uint64_t s = ((uint64_t)blockIdx.x * KM_READ_ITER + it) * 256u + threadIdx.x;
        if (s >= in.S) break;
        const unsigned long long key = in.tab[s], c = in.cnt[s];
        if (key == 0ull || c == 0ull) continue;
        acc[0] += 1ull; acc[1] += c; if (c > mx) mx = c;
        if (km_selected(in, c)) { acc[2] += 1ull; acc[3] += c; }
    }
    if (mx) atomicMax(&s_mx, mx);
    __syncthreads();
    if (threadIdx.x == 0u && s_mx) atomicMax(&st->c[4], s_mx);
    rows_sums_out<4>(acc, st->c);
}
// grid as k_kmers_count; hist, the lists and the index are zeroed in front of it on the stream, st->c[5] (the cursor) is 0.  The wave's scan is called by every lane.
__global__ void __launch_bounds__(256) k_kmers_write(KmersReadIn in, KmersReadStat* __restrict__ st) {
    __shared__ uint32_t km_hist[KM_HIST_LDS];
    const bool hist_lds = in.hist && in.hist_len <= KM_HIST_LDS;
    if (hist_lds) { for (uint32_t i = threadIdx.x; i < in.hist_len; i += 256u) km_hist[i] = 0u; }
    __syncthreads();
    if (blockIdx.x == 0u && threadIdx.x == 0u && in.ihdr) {
        in.ihdr->magic = SC_MAGIC; in.ihdr->version = SC_VERSION; in.ihdr->k = in.k; in.ihdr->S = in.iS; in.ihdr->flags = in.icollide ? SC_FLAG_COLLIDE : 0u;
    }
    unsigned long long claimed[1] = { 0ull };
    const bool list = in.values || in.counts;
    for (uint32_t it = 0; it < KM_READ_ITER; it++) {
        const uint64_t s0 = ((uint64_t)blockIdx.x * KM_READ_ITER + it) * 256u;
        if (s0 >= in.S) break;                                               // (the same in every thread)
        const uint64_t s = s0 + threadIdx.x;
        unsigned long long key = 0ull, c = 0ull;
        if (s < in.S) { key = in.tab[s]; c = in.cnt[s]; }
        const bool ent = key != 0ull && c != 0ull, sel = ent && km_selected(in, c);
        if (in.hist && ent) {
            const uint32_t bin = c - 1ull < (unsigned long long)(in.hist_len - 1u) ? (uint32_t)(c - 1ull) : in.hist_len - 1u;
            if (hist_lds) atomicAdd(&km_hist[bin], 1u); else atomicAdd(&in.hist[bin], 1ull);
        }
        if (list) {
            const uint32_t incl = wave_incl_sum<uint32_t>(sel ? 1u : 0u), tot = wave_last(incl);
            uint32_t lo = 0u, hi = 0u;
            if (lane_id() == 63 && tot) { const unsigned long long at = atomicAdd(&st->c[5], (unsigned long long)tot); lo = (uint32_t)at; hi = (uint32_t)(at >> 32); }
            lo = wave_last(lo); hi = wave_last(hi);
            const unsigned long long pos = (((unsigned long long)hi << 32) | lo) + incl - 1u;
            if (sel && pos < in.list_cap) {
                if (in.values) in.values[pos] = key & ~(1ull << 63);
                if (in.counts) in.counts[pos] = c;
            }
        }
        if (in.itab && sel) {
            const unsigned long long v = key & ~(1ull << 63); const uint64_t mask = in.iS - 1ull;
            if (sc_claim(in.itab, mask, sc_start(v, mask, in.icollide), sc_key(v), in.iS).claimed) claimed[0] += 1ull;
        }
    }
    if (hist_lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < in.hist_len; i += 256u) { const uint32_t v = km_hist[i]; if (v) atomicAdd(&in.hist[i], (unsigned long long)v); }
    }
    if (in.ihdr) rows_sums_out<4>(claimed, &in.ihdr->n_kmers);
}
