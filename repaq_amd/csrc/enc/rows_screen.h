// enc/rows_screen.h - reference sequences -> an exact set of canonical k-mers in a caller-owned index (rfq_screen_build), and rows against such an index -> the
// valid k-mers and the hits of every row, a keep byte per row and one summary (rfq_screen_rows): the step that asks WHAT a read is - contaminant removal, bait
// capture - beside rfq_judge_rows and rfq_dedup_rows.  It decides and moves no bytes.
// Part of rfq_encode_kernels.h (included from there, last, behind rows_lanes.h whose 16-byte pieces, group reductions, unit walk and sums it uses, and behind
// rows_adapter.h whose base classes - ar_bits, ar_cls - are the rule's; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the base bytes (include/rfq_hip.h has the rules).  A k-mer is 2 bits a base, the FIRST base in the highest bits; its canonical
// value is the smaller of itself and its reverse complement.  The index is a 64-byte header and S 64-bit slots: 0 = empty, else bit 63 | value; open addressing,
// linear probing, the start slot a multiplicative hash of the value (RFQ_SCREEN=collide: its four low bits - the header's flags say which, so that a lookup agrees
// with the build whatever the switch says later).
//   k_screen_refs              a lane per reference: the offsets are judged (they rise and end inside the blob), the bases summed.
//   k_screen_build             a lane per blob position: the k-mer there is valid when it lies inside ONE reference and is all A C G T; its canonical value is
//                              claimed with one atomicCAS on an empty slot (rows_dedup.h's claim loop; slots are read through dd_peek, never through a plain load).
//                              Byte by byte: the build is not hot.
//   k_screen_rows<16> / <64>   the common path: a row of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) / by a wave.  A lane loads ONE 16-byte
//                              group, turns it into 32 bits of classes and 16 valid bits (ar_bits), takes the next two lanes' words from registers (position 15
//                              with k = 31 reaches base 45: three words are always enough), forms its 16 forward values by funnel shifts, the reverse complements
//                              from the window reversed ONCE (bit reversal, pair swap, complement), validity from the 48 valid bits, and probes the set for every
//                              valid position.  LDS = true: the workgroup (1024 threads) copies the slots into LDS first and every probe is an LDS read.
//   k_screen_rows_long         any row length (and every call with RFQ_SCREEN=general): a wave per unit, tiles of 1024 bases; a tile's k-mers are formed when the
//                              NEXT tile's first two words are known, so a k-mer that straddles the seam is seen whole.
// A probe walk takes at most S steps whatever the slots hold.  All sums are integers and leave a workgroup as atomic adds: the same bits from run to run.
#define SC_NSUM 7                     // n_candidates, n_matched, n_kept, kmers, hits, bases_in, bases_kept
#define SC_BSUM 3                     // ref_bases (k_screen_refs); n_positions, n_kmers (k_screen_build)
#define SC_ITER 4u
#define SC_ERR_REFS 2u                // reference offsets that decrease or end past refs_len (RFQ_E_ARG); beside ROWS_ERR_LEN
#define SC_MAGIC 0x3158444E49435352ull        // "RSCINDX1"
#define SC_VERSION 1u
#define SC_FLAG_COLLIDE 1u
#define SC_K_MIN 4u
#define SC_K_MAX 31u
#define SC_LDS_SLOTS 16384u           // slots the LDS placement holds at most: 128 KiB of a compute unit's 160
#ifndef SC_LDS_NT
#define SC_LDS_NT 1024                // threads of a workgroup of the LDS placement (a multiple of 64; -DSC_LDS_NT=256 / 512 builds the shapes DESIGN.md compares it with)
#endif
struct ScreenHdr { unsigned long long magic; uint32_t version, k; unsigned long long S, n_kmers; uint32_t flags, pad[7]; };
static_assert(sizeof(ScreenHdr) == 64, "the index header is 64 bytes");
struct ScreenBuildIn {
    const uint8_t* blob; const unsigned long long* off;                       // ASCII references back to back, n_refs + 1 offsets
    uint64_t refs_len, n_refs;
    uint32_t k, collide;
    ScreenHdr* hdr; unsigned long long* tab; uint64_t S;                      // the index: header, S slots (zeroed per call)
};
struct ScreenIn {
    const uint8_t* b; const int32_t* lens; const uint8_t* cand;               // cand null: every unit is a candidate
    uint64_t total;                                                           // bytes of the row buffer: n_rows * row_len
    uint32_t n_rows, n_units, row_len;
    uint32_t vec_in;                                                          // row_len % 16 == 0 and the row buffer 16-byte aligned: a lane's group may be loaded whole
    uint32_t ascii, pairs, keep_matched, min_hits, min_pct;
    uint32_t k, collide;                                                      // of the index's header
    uint32_t steps;                                                           // common path: steps of a workgroup
    const unsigned long long* tab; uint64_t S;                                // the slots (a power of two)
    uint32_t* kmers; uint32_t* hits; uint8_t* keep;                           // [n_rows] each, or null
};
typedef RowsSums<SC_BSUM> ScreenBuildStat;
typedef RowsSums<SC_NSUM> ScreenStat;

// ---- the set
__device__ __forceinline__ uint64_t sc_start(unsigned long long v, uint64_t mask, uint32_t collide) {
    // (masked in BOTH forms: the flag and S come from the index's bytes, and a header with fewer than 16 slots passes the host's checks)
    return (collide ? (uint64_t)(v & 15ull) : (uint64_t)((v * 0x9E3779B97F4A7C15ull) >> 20)) & mask;
}
// v is in the set.  The table is complete and nobody writes it: plain loads (LDS or device memory).  At most S steps, whatever the slots hold.
__device__ __forceinline__ bool sc_probe(const unsigned long long* tab, uint64_t S, uint32_t collide, unsigned long long v) {
    const uint64_t mask = S - 1ull; const unsigned long long key = v | (1ull << 63);
    uint64_t s = sc_start(v, mask, collide);
    for (uint64_t n = 0; n < S; n++) {
        const unsigned long long cur = tab[s];
        if (cur == key) return true;
        if (cur == 0ull) return false;
        s = (s + 1ull) & mask;
    }
    return false;
}

// grid ceil(n_refs / 256) x 256 threads, a lane per reference
__global__ void __launch_bounds__(256) k_screen_refs(ScreenBuildIn in, ScreenBuildStat* __restrict__ st) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    unsigned long long acc[1] = { 0ull };
    if (r < in.n_refs) {
        const unsigned long long a = in.off[r], e = in.off[r + 1ull];
        if (e < a || e > in.refs_len) { atomicOr(&st->err, SC_ERR_REFS); atomicMin(&st->bad_row, (unsigned long long)r); }
        else acc[0] = e - a;
    }
    rows_sums_out<4>(acc, st->c);
}
// grid max(1, ceil(refs_len / 256)) x 256 threads, a lane per blob position, behind k_screen_refs on the stream: offsets it has refused are not followed.  The
// first thread writes the header (the slots and the header's count start at zero).  The walk ends: a reference of n bytes has at most n k-mers, the table twice
// as many slots as the blob has bytes.
__global__ void __launch_bounds__(256) k_screen_build(ScreenBuildIn in, ScreenBuildStat* __restrict__ st) {
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool ok = st->err == 0u;                                           // (the same in every thread: the kernel in front has ended)
    if (p == 0ull) { in.hdr->magic = SC_MAGIC; in.hdr->version = SC_VERSION; in.hdr->k = in.k; in.hdr->S = in.S; in.hdr->flags = in.collide ? SC_FLAG_COLLIDE : 0u; }
    unsigned long long acc[2] = { 0ull, 0ull };
    if (ok && p < in.refs_len && p + in.k <= in.refs_len) {
        // the reference p lies in: the last one that begins at or before p (empty references share their begin with the next one)
        uint64_t lo = 0, hi = in.n_refs + 1ull;
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (in.off[mid] <= p) lo = mid + 1ull; else hi = mid; }
        if (lo >= 1ull && lo <= in.n_refs && p + in.k <= in.off[lo]) {
            unsigned long long f = 0ull, rc = 0ull; bool valid = true;
            for (uint32_t i = 0; i < in.k; i++) {
                const uint32_t c = ar_cls(1u, in.blob[p + i]);
                if (c > 3u) { valid = false; break; }
                f = (f << 2) | c; rc |= (unsigned long long)(3u - c) << (2u * i);
            }
            if (valid) {
                const unsigned long long v = f < rc ? f : rc, key = v | (1ull << 63); const uint64_t mask = in.S - 1ull;
                uint64_t s = sc_start(v, mask, in.collide);
                acc[0] = 1ull;
                for (uint64_t n = 0; n < in.S; n++) {
                    unsigned long long cur = dd_peek(&in.tab[s]);
                    if (cur == 0ull) cur = atomicCAS(&in.tab[s], 0ull, key);
                    if (cur == 0ull) { acc[1] = 1ull; break; }              // (claimed: a value the set did not hold)
                    if (cur == key) break;
                    s = (s + 1ull) & mask;
                }
            }
        }
    }
    unsigned long long distinct[1] = { acc[1] };
    rows_sums_out<4>(acc, st->c + 1);
    rows_sums_out<4>(distinct, &in.hdr->n_kmers);
}

// ---- a lane's 16 positions
// the next lane's value in a group of LPR lanes (16: a DPP row, row_shl:1; 64: the wave, wave_shl:1); the group's last lane gets `fill`.  Called by ALL lanes of the wave.
#ifdef RFQ_SIMT_EMULATION
template <int LPR> __device__ __forceinline__ uint32_t grp_next(uint32_t v, uint32_t fill) {
    const uint32_t t = __shfl_down(v, 1u, LPR);
    return (lane_id() % LPR) == LPR - 1 ? fill : t;
}
__device__ __forceinline__ uint32_t sc_brev32(uint32_t x) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1); x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2); x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return bswap32(x);
}
#else
template <int LPR> __device__ __forceinline__ uint32_t grp_next(uint32_t v, uint32_t fill) {
    if constexpr (LPR == 16) return dpp_take<0x101, 0xF>(fill, v); else return dpp_take<0x130, 0xF>(fill, v);
}
__device__ __forceinline__ uint32_t sc_brev32(uint32_t x) { return __brev(x); }                   // v_bfrev_b32
#endif
// w: the classes of the lane's 16 positions, position j in bits 31 - 2j and 30 - 2j (the first base highest, like a k-mer's value); v: bit j = position j is one
// of A C G T and lies inside the read
struct ScLane { uint32_t w, v; };
// bit i of the 16 bits of x to bit 2i
__device__ __forceinline__ uint32_t sc_spread16(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu; x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}
__device__ __forceinline__ ScLane sc_lane(uint32_t ascii, const uint32_t (&b)[4], uint32_t span) {
    const ArBits m = ar_bits(ascii, b, span);
    ScLane r; r.w = (sc_spread16(ar_rev16(m.h)) << 1) | sc_spread16(ar_rev16(m.l)); r.v = m.v;
    return r;
}
// the 16 positions of w in reverse order, complemented
__device__ __forceinline__ uint32_t sc_rc32(uint32_t w) {
    const uint32_t x = sc_brev32(~w);
    return ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
}
// the 2k bits that begin t bits below the top of the 96 bits w0:w1:w2 (t + 2k <= 96)
__device__ __forceinline__ unsigned long long sc_win(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t t, uint32_t k) {
    const unsigned long long hi = ((unsigned long long)w0 << 32) | w1, lo = (unsigned long long)w2 << 32;
    const unsigned long long y = t == 0u ? hi : (t < 64u ? (hi << t) | (lo >> (64u - t)) : lo << (t - 64u));
    return y >> (64u - 2u * k);
}
// The k-mers that begin in lane a's 16 positions, b and c the next 32: valid ones, and those whose canonical value is in the set.  The reverse complement of the
// k-mer at j is the window of the reversed stream that begins at position 48 - j - k.
__device__ __forceinline__ void sc_count16(const ScreenIn& in, const unsigned long long* tab, const ScLane& a, const ScLane& b, const ScLane& c, uint32_t& kmers, uint32_t& hits) {
    if (!a.v) return;
    const uint32_t k = in.k;
    const unsigned long long V = (unsigned long long)a.v | ((unsigned long long)b.v << 16) | ((unsigned long long)c.v << 32), mk = (1ull << k) - 1ull;
    const uint32_t r0 = sc_rc32(c.w), r1 = sc_rc32(b.w), r2 = sc_rc32(a.w);
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        if (((V >> j) & mk) != mk) continue;
        const unsigned long long f = sc_win(a.w, b.w, c.w, 2u * j, k), rc = sc_win(r0, r1, r2, 2u * (48u - j - k), k);
        kmers++;
        hits += sc_probe(tab, in.S, in.collide, f < rc ? f : rc) ? 1u : 0u;
    }
}

// ---- a unit's verdict
__device__ __forceinline__ bool sc_cand(const ScreenIn& in, uint64_t u) {
    if (!in.cand) return true;
    return in.pairs ? (in.cand[2ull * u] != 0u && in.cand[2ull * u + 1ull] != 0u) : in.cand[u] != 0u;
}
// One lane per unit writes the unit's outputs and adds it to the sums it keeps for the workgroup (rk, rh: the rows' k-mers and hits; all 0 for no candidate).
__device__ __forceinline__ void sc_unit_out(const ScreenIn& in, uint64_t u, bool cand, const uint32_t (&rk)[2], const uint32_t (&rh)[2], unsigned long long lsum,
                                            unsigned long long (&acc)[SC_NSUM]) {
    const uint32_t nr = in.pairs ? 2u : 1u;
    const unsigned long long K = (unsigned long long)rk[0] + rk[1], H = (unsigned long long)rh[0] + rh[1];
    const bool matched = cand && H >= (in.min_hits > 1u ? in.min_hits : 1u) && 100ull * H >= (unsigned long long)in.min_pct * K;
    const bool keep = cand && (in.keep_matched ? matched : !matched);
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        if (in.kmers) in.kmers[g] = rk[i];
        if (in.hits) in.hits[g] = rh[i];
        if (in.keep) in.keep[g] = keep ? 1u : 0u;
    }
    if (cand) { acc[0] += 1ull; acc[1] += matched; acc[2] += keep; acc[3] += K; acc[4] += H; acc[5] += lsum; acc[6] += keep ? lsum : 0ull; }
}

// grid ceil(n_units / (NT / LPR * steps)) x NT threads (256; SC_LDS_NT with the table in LDS: S * 8 bytes of dynamic LDS).  A group of the workgroup (UnitGroup:
// LPR lanes, NT / LPR groups) takes a unit per step, in.steps steps, one row after the other.  ALL rows' lengths are checked, candidates or not; only a candidate's
// bytes are loaded.  What depends on the unit only masks: the lane moves and the reductions are called by every lane of the wave.
template <int LPR, int NT, bool LDS> __global__ void __launch_bounds__(NT) k_screen_rows(ScreenIn in, ScreenStat* __restrict__ st) {
    const UnitGroup<LPR> ug{};
    constexpr uint32_t R = (uint32_t)NT / LPR;
    const unsigned long long* tab = in.tab;
    if constexpr (LDS) {
        // (the interpreter's buffer for dynamic LDS holds 64 KB: there the slots get a block of the kernel's own, of the size the host never exceeds)
#ifdef RFQ_SIMT_EMULATION
        __shared__ ulonglong2 sc_lds[SC_LDS_SLOTS / 2u];
#else
        RFQ_DYN_SHARED(ulonglong2, sc_lds);
#endif
        for (uint32_t i = threadIdx.x; i < (uint32_t)(in.S / 2u); i += (uint32_t)NT) sc_lds[i] = ((const ulonglong2*)in.tab)[i];        // (S is even, the slots 16-byte aligned)
        __syncthreads();
        tab = (const unsigned long long*)sc_lds;
    }
    const uint32_t nr = in.pairs ? 2u : 1u;
    unsigned long long acc[SC_NSUM] = {};
    for (uint32_t it = 0; it < in.steps; it++) {
        const uint64_t u = ((uint64_t)blockIdx.x * in.steps + it) * R + ug.grp;
        if (ug.past(u, in.n_units)) break;
        const bool live = u < in.n_units, cand = live && sc_cand(in, u);
        uint32_t rk[2] = { 0u, 0u }, rh[2] = { 0u, 0u }; unsigned long long lsum = 0ull;
        for (uint32_t i = 0; i < nr; i++) {
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u;
            uint32_t b[4] = { 0u, 0u, 0u, 0u };
            const bool mine = cand && ug.x0 < l;
            if (mine) rows_ld16(in.b, in.vec_in, in.total, g * in.row_len, ug.x0, l, b);
            const ScLane a = sc_lane(in.ascii, b, mine ? rows_span(ug.x0, 0u, l) : 0u);
            ScLane n1, n2;
            n1.w = grp_next<LPR>(a.w, 0u); n1.v = grp_next<LPR>(a.v, 0u); n2.w = grp_next<LPR>(n1.w, 0u); n2.v = grp_next<LPR>(n1.v, 0u);
            uint32_t nk = 0u, nh = 0u;
            sc_count16(in, tab, a, n1, n2, nk, nh);
            const uint32_t t = grp_sum<LPR>(nk | (nh << 16));                // (a row of the common path has at most 1024 positions)
            rk[i] = t & 0xFFFFu; rh[i] = t >> 16; lsum += l;
        }
        if (ug.gl == 0u && live) sc_unit_out(in, u, cand, rk, rh, lsum, acc);
    }
    rows_sums_out<NT / 64>(acc, st->c);
}

// ---- any row length
// the next lane's value in the wave, lane 63 gets `fill` (the first lane's value of the tile behind)
__device__ __forceinline__ ScLane sc_next64(const ScLane& x, uint32_t fw, uint32_t fv) { ScLane r; r.w = grp_next<64>(x.w, fw); r.v = grp_next<64>(x.v, fv); return r; }
// grid n_units x 64 threads: a wave per unit, everything about the unit is the same in every lane.  Tiles of 1024 positions from the row's start; the k-mers that
// begin in a tile are formed one step later, when lanes 62 and 63 can take the next tile's first two words.  A lane adds up its positions' counts over the tiles, one
// reduction per row.
__global__ void __launch_bounds__(64) k_screen_rows_long(ScreenIn in, ScreenStat* __restrict__ st) {
    const uint64_t u = blockIdx.x; const uint32_t x0 = 16u * threadIdx.x, nr = in.pairs ? 2u : 1u;
    const bool cand = sc_cand(in, u);
    unsigned long long acc[SC_NSUM] = {};
    uint32_t rk[2] = { 0u, 0u }, rh[2] = { 0u, 0u }; unsigned long long lsum = 0ull;
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u);
        const uint64_t rowbase = g * in.row_len;
        uint32_t nk = 0u, nh = 0u;
        ScLane prev; prev.w = prev.v = 0u;
        if (cand) for (uint64_t t0 = 0; t0 < (uint64_t)l + 1024u; t0 += 1024u) {        // (one step behind the last tile: its k-mers)
            ScLane cur; cur.w = cur.v = 0u;
            const uint64_t p0 = t0 + x0;
            if (p0 < l) {
                uint32_t b[4];
                rows_ld16(in.b, in.vec_in, in.total, rowbase, (uint32_t)p0, l, b);
                cur = sc_lane(in.ascii, b, rows_span((uint32_t)p0, 0u, l));
            }
            const uint32_t w0 = wave_read(cur.w, 0u), v0 = wave_read(cur.v, 0u), w1 = wave_read(cur.w, 1u), v1 = wave_read(cur.v, 1u);
            const ScLane n1 = sc_next64(prev, w0, v0), n2 = sc_next64(n1, w1, v1);
            sc_count16(in, in.tab, prev, n1, n2, nk, nh);
            prev = cur;
        }
        const unsigned long long t = wave_sum<unsigned long long>((unsigned long long)nk | ((unsigned long long)nh << 32));
        rk[i] = (uint32_t)t; rh[i] = (uint32_t)(t >> 32); lsum += l;
    }
    if (threadIdx.x == 0u) sc_unit_out(in, u, cand, rk, rh, lsum, acc);
    rows_sums_out<1>(acc, st->c);
}
