// enc/rows_kmer_lanes.h - what the rows kernels that work on bases 2 bits at a time share: a lane's 16 positions as 2-bit classes, the canonical k-mers that begin
// in them, the row of the common path and the walk over a row of any length that form them, and the set of 64-bit slots the values are looked up and claimed in
// (rfq_screen_build / rfq_screen_rows, rfq_kmers_rows / rfq_kmers_read; rfq_demux_rows takes the classes and the window, rfq_dedup_rows the slot read).
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose 16-byte loads, spans and UnitGroup it uses and behind rows_adapter.h whose base
// classes - ar_bits, ar_cls - are the rule's; in front of rows_dedup.h, rows_screen.h, rows_kmers.h and rows_demux.h, in any order; not a stand-alone header).
#pragma once
// ---- the set: S 64-bit slots (S a power of two), 0 = empty, else bit 63 | value; open addressing, linear probing, every slot number masked to S.  As a screen
// index (rfq_screen_build and rfq_kmers_read write one, rfq_screen_rows reads it) the slots lie behind this header
#define SC_MAGIC 0x3158444E49435352ull        // "RSCINDX1"
#define SC_VERSION 1u
#define SC_FLAG_COLLIDE 1u
struct ScreenHdr { unsigned long long magic; uint32_t version, k; unsigned long long S, n_kmers; uint32_t flags, pad[7]; };
static_assert(sizeof(ScreenHdr) == 64, "the index header is 64 bytes");
__device__ __forceinline__ unsigned long long sc_key(unsigned long long v) { return v | (1ull << 63); }
// A slot that other lanes may claim meanwhile is read through the compare-and-swap's return value or through this relaxed agent-scope atomic load and never through
// a plain load: another compute unit's claim is visible in the L2, not in this one's vector L1.  A slot never changes once it is claimed.
__device__ __forceinline__ unsigned long long slot_peek(const unsigned long long* p) {
#ifdef RFQ_SIMT_EMULATION
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// the slot a walk for v starts at: a multiplicative hash of the value (collide: its four low bits - the tests' form with long chains)
__device__ __forceinline__ uint64_t sc_start(unsigned long long v, uint64_t mask, uint32_t collide) {
    // (masked in BOTH forms: the flag and S come from the index's bytes, and a header with fewer than 16 slots passes the host's checks)
    return (collide ? (uint64_t)(v & 15ull) : (uint64_t)((v * 0x9E3779B97F4A7C15ull) >> 20)) & mask;
}
// v is in the set.  The table is complete and nobody writes it: plain loads (LDS or device memory).  At most S steps, whatever the slots hold.
__device__ __forceinline__ bool sc_probe(const unsigned long long* tab, uint64_t S, uint32_t collide, unsigned long long v) {
    const uint64_t mask = S - 1ull; const unsigned long long key = sc_key(v);
    uint64_t s = sc_start(v, mask, collide);
    for (uint64_t n = 0; n < S; n++) {
        const unsigned long long cur = tab[s];
        if (cur == key) return true;
        if (cur == 0ull) return false;
        s = (s + 1ull) & mask;
    }
    return false;
}
// The claim: from slot s on, at most `bound` steps (N: the bound's type - a 32-bit bound keeps a 32-bit counter), the slot that holds `key` - an empty one is claimed
// with one atomicCAS, and `claimed` says that THIS call did so: the set did not hold the key.  SC_NO_SLOT: the walk met neither the key nor an empty slot.  No
// waiting anywhere.  (k_dedup_claim's loop stays its own: it compares a tag and then the rows' bytes and has no bound.  The LDS stage of km_add stays its own: 32-bit
// slot numbers, a volatile LDS read, and a miss there is no loss.)
#define SC_NO_SLOT 0xFFFFFFFFFFFFFFFFull
struct ScSlot { uint64_t s; bool claimed; };
template <class N> __device__ __forceinline__ ScSlot sc_claim(unsigned long long* tab, uint64_t mask, uint64_t s, unsigned long long key, N bound) {
    for (N n = 0; n < bound; n++) {
        unsigned long long cur = slot_peek(&tab[s]);
        if (cur == 0ull) { cur = atomicCAS(&tab[s], 0ull, key); if (cur == 0ull) return { s, true }; }
        if (cur == key) return { s, false };
        s = (s + 1ull) & mask;
    }
    return { SC_NO_SLOT, false };
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
// the next lane's value in the wave, lane 63 gets `fill` (the first lane's value of the tile behind)
__device__ __forceinline__ ScLane sc_next64(const ScLane& x, uint32_t fw, uint32_t fv) { ScLane r; r.w = grp_next<64>(x.w, fw); r.v = grp_next<64>(x.v, fv); return r; }

// ---- the k-mers of a lane, of a row
// The k-mers that begin in lane a's 16 positions, b and c the next 32 (position 15 with k = 31 reaches base 45: three words are always enough): visit(value) is
// called with the canonical value of every valid one - all A C G T, inside the read: the 48 valid bits -; returns their number.  The forward values are funnel
// shifts; the reverse complement of the k-mer at j is the window of the reversed stream (bit reversal, pair swap, complement: ONCE) that begins at position
// 48 - j - k.  visit is a lambda of the caller's, inlined.
// UNROLL is the count `#pragma unroll` gets for the 16 positions, and the two callers differ on purpose: the screen's visit is one probe walk and its loop is
// unrolled whole (16: constant shifts in every window, about 3100 static instructions a kernel); the count's visit is the add with its LDS and device-memory walks,
// which 16 copies of would only bloat - it stays the loop it is (1: about 1050 instructions).
template <int UNROLL, class F> __device__ __forceinline__ uint32_t sc_kmers16(uint32_t k, const ScLane& a, const ScLane& b, const ScLane& c, F&& visit) {
    if (!a.v) return 0u;
    uint32_t kmers = 0u;
    const unsigned long long V = (unsigned long long)a.v | ((unsigned long long)b.v << 16) | ((unsigned long long)c.v << 32), mk = (1ull << k) - 1ull;
    const uint32_t r0 = sc_rc32(c.w), r1 = sc_rc32(b.w), r2 = sc_rc32(a.w);
#pragma unroll UNROLL
    for (uint32_t j = 0; j < 16u; j++) {
        if (((V >> j) & mk) != mk) continue;
        const unsigned long long f = sc_win(a.w, b.w, c.w, 2u * j, k), rc = sc_win(r0, r1, r2, 2u * (48u - j - k), k);
        kmers++;
        visit(f < rc ? f : rc);
    }
    return kmers;
}
// Row g of checked length l on the common path (In: the call's block - b, vec_in, total, row_len, ascii, k), held by the group ug: the lane loads ONE 16-byte group
// (only where `wanted`: the row's bytes are the call's to read), takes the next two lanes' words from registers and visits its positions' k-mers; returns the
// lane's count.  What depends on the row only masks: the lane moves in here are called by EVERY lane of the wave, wanted or not, live or not (l = 0).
template <int UNROLL, int LPR, class In, class F> __device__ __forceinline__ uint32_t sc_kmers_row(const In& in, const UnitGroup<LPR>& ug, uint64_t g, uint32_t l, bool wanted, F&& visit) {
    uint32_t b[4] = { 0u, 0u, 0u, 0u };
    const bool mine = wanted && ug.x0 < l;
    if (mine) rows_ld16(in.b, in.vec_in, in.total, g * in.row_len, ug.x0, l, b);
    const ScLane a = sc_lane(in.ascii, b, mine ? rows_span(ug.x0, 0u, l) : 0u);
    ScLane n1, n2;
    n1.w = grp_next<LPR>(a.w, 0u); n1.v = grp_next<LPR>(a.v, 0u); n2.w = grp_next<LPR>(n1.w, 0u); n2.v = grp_next<LPR>(n1.v, 0u);
    return sc_kmers16<UNROLL>(in.k, a, n1, n2, visit);
}
// Row g of any length l, walked by a wave (64 threads a workgroup; called by all of them with the same g, l and `wanted`: nothing of a row that is not is read):
// tiles of 1024 positions from the row's start.  The k-mers that begin in a tile are formed one step later, when lanes 62 and 63 can take the next tile's first two
// words - a k-mer that straddles the seam is seen whole -, hence the one step behind the last tile.  Returns the lane's count over all tiles.
template <int UNROLL, class In, class F> __device__ __forceinline__ uint32_t sc_kmers_row_long(const In& in, uint64_t g, uint32_t l, bool wanted, F&& visit) {
    const uint32_t x0 = 16u * threadIdx.x; const uint64_t rowbase = g * in.row_len;
    uint32_t nk = 0u;
    ScLane prev; prev.w = prev.v = 0u;
    if (wanted) for (uint64_t t0 = 0; t0 < (uint64_t)l + 1024u; t0 += 1024u) {
        ScLane cur; cur.w = cur.v = 0u;
        const uint64_t p0 = t0 + x0;
        if (p0 < l) {
            uint32_t b[4];
            rows_ld16(in.b, in.vec_in, in.total, rowbase, (uint32_t)p0, l, b);
            cur = sc_lane(in.ascii, b, rows_span((uint32_t)p0, 0u, l));
        }
        const uint32_t w0 = wave_read(cur.w, 0u), v0 = wave_read(cur.v, 0u), w1 = wave_read(cur.w, 1u), v1 = wave_read(cur.v, 1u);
        const ScLane n1 = sc_next64(prev, w0, v0), n2 = sc_next64(n1, w1, v1);
        nk += sc_kmers16<UNROLL>(in.k, prev, n1, n2, visit);
        prev = cur;
    }
    return nk;
}
