// enc/rows_dedup.h - rows -> a keep byte per row that leaves ONE unit (a row, or a pair of rows) of every class of units with identical keys, the representative
// and the size of every class, a class-size histogram and one summary (rfq_dedup_rows): the step between rfq_judge_rows and rfq_select_rows that relates rows to
// each other.  It decides and moves no bytes.
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose 16-byte pieces, group reductions, unit walk and candidate test it uses, and behind
// rows_kmer_lanes.h for its slot read slot_peek; not a stand-alone header).
#pragma once
// A key is (k, bytes [0, k)) of a row, k = min(length, key_len); a pair's key is R1's followed by R2's (include/rfq_hip.h has the rules).  Three kernels:
//   k_dedup_key<16> / <64>   a unit of rows of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) / by a wave, a lane loads ONE 16-byte group of the
//   k_dedup_key_long         bases (and of the scores in BEST_QUAL) - any row length: a wave per unit walks the rows in tiles of 1024 bytes.  Per unit: the
//                            length check, candidacy, a 64-bit fingerprint of the key and the score (the sum of the scores over the key window), into scratch; per
//                            batch n_candidates and bases_in, into the verdict block.
//   k_dedup_claim            a lane per candidate unit finds its class's slot in a table of S 64-bit words (open addressing, linear probing): an empty slot is
//                            claimed with one atomicCAS, a foreign slot with my tag is compared byte by byte with its claimant's rows - equal: it is my class.
//                            On the class's slot one atomicMax (the representative) and one atomicAdd (the size).  No waiting anywhere: every step is wait-free.
//   k_dedup_resolve          a lane per unit reads its slot's representative and size and writes keep, dup_of, count; the histogram through an LDS copy per
//                            workgroup, the sums reduced per workgroup first.
// The fingerprint is private: it picks the slot a probe starts at and the tag that saves byte compares, and NOTHING ELSE - equality is always decided on the bytes,
// and what a class reports (its lowest member or its best one, its size) is the same whichever member claimed the slot and in whatever order the others came.  All
// sums are integers.  RFQ_DEDUP=collide keeps 4 bits of the fingerprint: every probe chain is long and every tag hit a real compare (the tests' "general" form).
#define DD_NSUM 5                     // n_candidates, bases_in (k_dedup_key); n_classes, bases_kept (k_dedup_resolve); [4] max_class (an atomicMax)
#define DD_ITER 8u
#define DD_NONE 0xFFFFFFFFu           // in the score scratch: not a candidate; in the slot scratch: no slot
#define DD_HIST_MAX 1024u
struct DedupIn {
    const uint8_t* b; const uint8_t* q; const int32_t* lens; const uint8_t* cand;     // q null: FIRST (no score); cand null: every unit is a candidate
    uint64_t total;                                                           // bytes of a row buffer: n_rows * row_len
    uint32_t n_rows, n_units, row_len;
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffers 16-byte aligned: a lane's group may be loaded whole
    uint32_t pairs, key_len, collide;
    uint32_t hist_len;
    unsigned long long* fp; uint32_t* score; uint32_t* slot;                  // [n_units] scratch: fingerprint, score (DD_NONE: no candidate), the class's slot
    unsigned long long* tab; unsigned long long* best; uint32_t* cnt;         // [S] the table, zeroed per call
    uint64_t S;                                                               // a power of two, >= 2 * n_units
    uint8_t* keep; int32_t* dup_of; uint32_t* count; unsigned long long* hist;        // [n_rows], [n_units], [n_units], [hist_len], or null
};
typedef RowsSums<DD_NSUM> DedupStat;

// the key window of a row of l bytes
__device__ __forceinline__ uint32_t dd_kwin(const DedupIn& in, uint32_t l) { return in.key_len && in.key_len < l ? in.key_len : l; }
// ---- the fingerprint: the sum over a key's 16-byte groups of mix(group bytes, group index) - a sum, so that the lanes' parts combine with row_sum / wave_sum in
// any order -, then the length folded in; groups that hold no key byte add nothing, so the value is a function of the key alone.
__device__ __forceinline__ unsigned long long dd_avalanche(unsigned long long x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}
__device__ __forceinline__ unsigned long long dd_mix16(const uint32_t (&w)[4], uint32_t gi) {
    const unsigned long long a = ((unsigned long long)w[1] << 32) | w[0], b = ((unsigned long long)w[3] << 32) | w[2];
    unsigned long long x = (a ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(gi + 1u))) * 0xD6E8FEB86659FD93ull;
    x ^= x >> 32;
    x = (x + b) * 0xA0761D6478BD642Full;
    return x ^ (x >> 29);
}
__device__ __forceinline__ unsigned long long dd_fold_len(unsigned long long sum, uint32_t k) { return dd_avalanche(sum ^ (0x8EBC6AF09C88C6E3ull * (unsigned long long)(k + 1u))); }
// R2's fingerprint into R1's: not symmetric, so that a pair with its mates swapped gets another value
__device__ __forceinline__ unsigned long long dd_fold_mate(unsigned long long f1, unsigned long long f2) { return dd_avalanche(f1 * 0x9FB21C651E98DF25ull + ((f2 << 23) | (f2 >> 41))); }

// one lane per unit: the unit's scratch entries and its part of the sums
__device__ __forceinline__ void dd_key_out(const DedupIn& in, uint64_t u, bool cand, unsigned long long fp, uint32_t score, unsigned long long lsum, unsigned long long (&acc)[2]) {
    in.fp[u] = fp; in.score[u] = cand ? score : DD_NONE;
    if (cand) { acc[0] += 1ull; acc[1] += lsum; }
}

// grid ceil(n_units / (256 / LPR * DD_ITER)) x 256 threads.  A group of the workgroup (UnitGroup: LPR lanes) takes a unit per step, DD_ITER steps, one row after
// the other.  ALL rows' lengths are checked, candidates or not; only a candidate's bytes are loaded.  What depends on the unit only masks:
// the reductions are called by every lane of the wave.
template <int LPR> __global__ void __launch_bounds__(256) k_dedup_key(DedupIn in, DedupStat* __restrict__ st) {
    const UnitGroup<LPR> ug{};
    const uint32_t nr = in.pairs ? 2u : 1u;
    unsigned long long acc[2] = { 0ull, 0ull };
    for (uint32_t it = 0; it < DD_ITER; it++) {
        const uint64_t u = ug.unit(it, DD_ITER);
        if (ug.past(u, in.n_units)) break;
        const bool live = u < in.n_units, cand = live && rows_cand(in, u);
        unsigned long long fp = 0ull, lsum = 0ull; uint32_t score = 0u;
        for (uint32_t i = 0; i < nr; i++) {
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u, k = dd_kwin(in, l);
            const uint64_t rowbase = g * in.row_len;
            uint32_t b[4] = { 0u, 0u, 0u, 0u }, q[4] = { 0u, 0u, 0u, 0u };
            const bool mine = cand && ug.x0 < k;
            if (mine) { rows_ld16(in.b, in.vec_in, in.total, rowbase, ug.x0, k, b); if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, ug.x0, k, q); }
            const unsigned long long hs = grp_sum<LPR>(mine ? dd_mix16(b, ug.gl) : 0ull);
            const uint32_t sc = grp_sum<LPR>(rows_sum16(q));
            const unsigned long long f = dd_fold_len(hs, k);
            fp = i == 0u ? f : dd_fold_mate(fp, f);
            score += sc; lsum += l;
        }
        if (ug.gl == 0u && live) dd_key_out(in, u, cand, fp, score, lsum, acc);
    }
    rows_sums_out<4>(acc, st->c);
}
// grid n_units x 64 threads: a wave per unit, everything about the unit is the same in every lane.  A lane adds up its groups' parts over the tiles, one reduction
// per row.
__global__ void __launch_bounds__(64) k_dedup_key_long(DedupIn in, DedupStat* __restrict__ st) {
    const uint64_t u = blockIdx.x; const uint32_t x0 = 16u * threadIdx.x, nr = in.pairs ? 2u : 1u;
    const bool cand = rows_cand(in, u);
    unsigned long long acc[2] = { 0ull, 0ull };
    unsigned long long fp = 0ull, lsum = 0ull; uint32_t score = 0u;
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u), k = dd_kwin(in, l);
        const uint64_t rowbase = g * in.row_len;
        unsigned long long h = 0ull; uint32_t s = 0u;
        if (cand) for (uint32_t t0 = 0; t0 < k; t0 += 1024u) {
            const uint32_t p0 = t0 + x0;
            if (p0 >= k) continue;
            uint32_t b[4], q[4] = { 0u, 0u, 0u, 0u };
            rows_ld16(in.b, in.vec_in, in.total, rowbase, p0, k, b);
            if (in.q) rows_ld16(in.q, in.vec_in, in.total, rowbase, p0, k, q);
            h += dd_mix16(b, p0 >> 4); s += rows_sum16(q);
        }
        const unsigned long long f = dd_fold_len(wave_sum<unsigned long long>(h), k);
        fp = i == 0u ? f : dd_fold_mate(fp, f);
        score += wave_sum<uint32_t>(s); lsum += l;
    }
    if (threadIdx.x == 0u) dd_key_out(in, u, cand, fp, score, lsum, acc);
    rows_sums_out<1>(acc, st->c);
}

// ---- the table.  A slot is tag32 << 32 | (unit + 1), 0 = empty.  It is read through the compare-and-swap's return value or through slot_peek and never through a
// plain load.  A slot never changes once it is claimed.
// the keys of units u and v are equal: lengths first, then the bytes 16 at a time (the rows are read-only input of the call: nothing needs ordering)
__device__ __forceinline__ bool dd_same(const DedupIn& in, uint64_t u, uint64_t v) {
    const uint32_t nr = in.pairs ? 2u : 1u;
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i), h = rows_unit_row(in.pairs, v, i);
        const uint32_t k = dd_kwin(in, rows_len_or0(in, g));       // (the key kernel has reported a bad length already)
        if (k != dd_kwin(in, rows_len_or0(in, h))) return false;
        const uint64_t gb = g * in.row_len, hb = h * in.row_len;
        for (uint32_t off = 0; off < k; off += 16u) {
            uint32_t a[4], c[4];
            rows_ld16(in.b, in.vec_in, in.total, gb, off, k, a); rows_ld16(in.b, in.vec_in, in.total, hb, off, k, c);
            if ((a[0] ^ c[0]) | (a[1] ^ c[1]) | (a[2] ^ c[2]) | (a[3] ^ c[3])) return false;
        }
    }
    return true;
}
// grid ceil(n_units / 256) x 256 threads, a lane per unit.  The walk ends: the table has at least twice as many slots as there are units, and every unit claims at
// most one.  Whoever claimed a class's slot, every member arrives at it: members probe the same chain from the same start, and a slot, once claimed, stays.
// (Not sc_claim: a slot here is a tag and its claimant, equality is decided on the rows' bytes, and the walk has no bound.)
__global__ void __launch_bounds__(256) k_dedup_claim(DedupIn in) {
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (u >= in.n_units) return;
    const uint32_t score = in.score[u];
    if (score == DD_NONE) { in.slot[u] = DD_NONE; return; }
    unsigned long long fp = in.fp[u];
    if (in.collide) fp = (fp & 15ull) | ((fp & 15ull) << 32);
    const uint64_t mask = in.S - 1ull;
    const unsigned long long tag = fp >> 32, mine = (tag << 32) | (unsigned long long)(u + 1ull);
    uint64_t s = (uint64_t)(fp * 0x9E3779B97F4A7C15ull >> 20) & mask;
    if (in.collide) s = fp & 15ull;
    for (;;) {
        unsigned long long cur = slot_peek(&in.tab[s]);
        if (cur == 0ull) cur = atomicCAS(&in.tab[s], 0ull, mine);
        if (cur == 0ull) break;                                             // (claimed: the slot is my class's, and I am its first member)
        if ((cur >> 32) == tag && dd_same(in, u, (uint64_t)(uint32_t)cur - 1ull)) break;
        s = (s + 1ull) & mask;
    }
    // "the highest score, then the lowest index" as one maximum (score 0 in FIRST: the lowest index); the order of arrival changes neither
    atomicMax(&in.best[s], ((unsigned long long)score << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)u));
    atomicAdd(&in.cnt[s], 1u);
    in.slot[u] = (uint32_t)s;
}

// grid ceil(n_units / 256) x 256 threads, a lane per unit (the table is complete: the claim kernel has ended).
__global__ void __launch_bounds__(256) k_dedup_resolve(DedupIn in, DedupStat* __restrict__ st) {
    __shared__ uint32_t s_hist[DD_HIST_MAX];
    __shared__ uint32_t s_max[4];
    const uint64_t u = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = u < in.n_units;
    const bool hist = in.hist != nullptr;                                    // (uniform)
    if (hist) { for (uint32_t i = threadIdx.x; i < in.hist_len; i += 256u) s_hist[i] = 0u; __syncthreads(); }
    unsigned long long acc[2] = { 0ull, 0ull }; uint32_t mx = 0u;
    if (live) {
        const uint32_t s = in.slot[u];
        uint32_t rep = DD_NONE, c = 0u;
        if (s != DD_NONE) { rep = 0xFFFFFFFFu - (uint32_t)in.best[s]; c = in.cnt[s]; }
        const bool is_rep = s != DD_NONE && rep == (uint32_t)u;
        const uint32_t nr = in.pairs ? 2u : 1u; unsigned long long lsum = 0ull;
        for (uint32_t i = 0; i < nr; i++) {
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            if (in.keep) in.keep[g] = is_rep ? 1u : 0u;
            if (is_rep) lsum += rows_len_or0(in, g);
        }
        if (in.dup_of) in.dup_of[u] = s != DD_NONE ? (int32_t)rep : -1;
        if (in.count) in.count[u] = is_rep ? c : 0u;
        if (is_rep) {
            acc[0] = 1ull; acc[1] = lsum; mx = c;
            if (hist) atomicAdd(&s_hist[(c < in.hist_len ? c : in.hist_len) - 1u], 1u);
        }
    }
    rows_sums_out<4>(acc, st->c + 2);
    mx = wave_max<uint32_t>(mx);
    if (lane_id() == 0) s_max[wave_id()] = mx;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t m = s_max[0];
        for (int w = 1; w < 4; w++) m = s_max[w] > m ? s_max[w] : m;
        if (m) atomicMax(&st->c[4], (unsigned long long)m);
    }
    if (hist) for (uint32_t i = threadIdx.x; i < in.hist_len; i += 256u) { const uint32_t v = s_hist[i]; if (v) atomicAdd(&in.hist[i], (unsigned long long)v); }
}
