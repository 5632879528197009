// enc/rows_screen.h - reference sequences -> an exact set of canonical k-mers in a caller-owned index (rfq_screen_build), and rows against such an index -> the
// valid k-mers and the hits of every row, a keep byte per row and one summary (rfq_screen_rows): the step that asks WHAT a read is - contaminant removal, bait
// capture - beside rfq_judge_rows and rfq_dedup_rows.  It decides and moves no bytes.
// Part of rfq_encode_kernels.h (included from there, behind rows_lanes.h whose group reductions, unit walk, candidate test and sums it uses, behind rows_adapter.h
// whose base class ar_cls is the build's, and behind rows_kmer_lanes.h, which has the set - the slot format, sc_start, sc_probe, sc_claim - and the k-mers of a
// row - sc_kmers_row, sc_kmers_row_long; not a stand-alone header).
#pragma once
// Everything is integer arithmetic on the base bytes (include/rfq_hip.h has the rules).  A k-mer is 2 bits a base, the FIRST base in the highest bits; its canonical
// value is the smaller of itself and its reverse complement.  The index is a 64-byte header and S 64-bit slots: 0 = empty, else bit 63 | value; open addressing,
// linear probing, the start slot a multiplicative hash of the value (RFQ_SCREEN=collide: its four low bits - the header's flags say which, so that a lookup agrees
// with the build whatever the switch says later).
//   k_screen_refs              a lane per reference: the offsets are judged (they rise and end inside the blob), the bases summed.
//   k_screen_build             a lane per blob position: the k-mer there is valid when it lies inside ONE reference and is all A C G T; its canonical value is
//                              claimed with one atomicCAS on an empty slot (sc_claim: slots are read through slot_peek, never through a plain load).
//                              Byte by byte: the build is not hot.
//   k_screen_rows<16> / <64>   the common path: a row of up to 256 / 1024 bytes is held by a group of 16 lanes (a DPP row) / by a wave; a lane forms the k-mers
//                              of its 16 positions (sc_kmers_row) and probes the set for every valid one.  LDS = true: the workgroup (1024 threads) copies the
//                              slots into LDS first and every probe is an LDS read.
//   k_screen_rows_long         any row length (and every call with RFQ_SCREEN=general): a wave per unit, tiles of 1024 bases (sc_kmers_row_long).
// A probe walk takes at most S steps whatever the slots hold.  All sums are integers and leave a workgroup as atomic adds: the same bits from run to run.
#define SC_NSUM 7                     // n_candidates, n_matched, n_kept, kmers, hits, bases_in, bases_kept
#define SC_BSUM 3                     // ref_bases (k_screen_refs); n_positions, n_kmers (k_screen_build)
#define SC_ITER 4u
#define SC_ERR_REFS 2u                // reference offsets that decrease or end past refs_len (RFQ_E_ARG); beside ROWS_ERR_LEN
#define SC_K_MIN 4u
#define SC_K_MAX 31u
#define SC_LDS_SLOTS 16384u           // slots the LDS placement holds at most: 128 KiB of a compute unit's 160
#ifndef SC_LDS_NT
#define SC_LDS_NT 1024                // threads of a workgroup of the LDS placement (a multiple of 64; -DSC_LDS_NT=256 / 512 builds the shapes DESIGN.md compares it with)
#endif
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
                const unsigned long long v = f < rc ? f : rc; const uint64_t mask = in.S - 1ull;
                acc[0] = 1ull;
                if (sc_claim(in.tab, mask, sc_start(v, mask, in.collide), sc_key(v), in.S).claimed) acc[1] = 1ull;       // (a value the set did not hold)
            }
        }
    }
    unsigned long long distinct[1] = { acc[1] };
    rows_sums_out<4>(acc, st->c + 1);
    rows_sums_out<4>(distinct, &in.hdr->n_kmers);
}

// ---- a unit's verdict
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
// bytes are loaded.  What depends on the unit only masks: the lane moves (inside sc_kmers_row) and the reductions are called by every lane of the wave.
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
        const bool live = u < in.n_units, cand = live && rows_cand(in, u);
        uint32_t rk[2] = { 0u, 0u }, rh[2] = { 0u, 0u }; unsigned long long lsum = 0ull;
        for (uint32_t i = 0; i < nr; i++) {
            const uint64_t g = rows_unit_row(in.pairs, u, i);
            const uint32_t l = live ? rows_len_checked(in, g, st, ug.gl == 0u) : 0u;
            uint32_t nh = 0u;
            const uint32_t nk = sc_kmers_row<16>(in, ug, g, l, cand, [&](unsigned long long v) __attribute__((always_inline)) { nh += sc_probe(tab, in.S, in.collide, v) ? 1u : 0u; });
            const uint32_t t = grp_sum<LPR>(nk | (nh << 16));                // (a row of the common path has at most 1024 positions)
            rk[i] = t & 0xFFFFu; rh[i] = t >> 16; lsum += l;
        }
        if (ug.gl == 0u && live) sc_unit_out(in, u, cand, rk, rh, lsum, acc);
    }
    rows_sums_out<NT / 64>(acc, st->c);
}

// ---- any row length
// grid n_units x 64 threads: a wave per unit, everything about the unit is the same in every lane.  A lane adds up its positions' counts over the tiles of
// sc_kmers_row_long, one reduction per row.
__global__ void __launch_bounds__(64) k_screen_rows_long(ScreenIn in, ScreenStat* __restrict__ st) {
    const uint64_t u = blockIdx.x; const uint32_t nr = in.pairs ? 2u : 1u;
    const bool cand = rows_cand(in, u);
    unsigned long long acc[SC_NSUM] = {};
    uint32_t rk[2] = { 0u, 0u }, rh[2] = { 0u, 0u }; unsigned long long lsum = 0ull;
    for (uint32_t i = 0; i < nr; i++) {
        const uint64_t g = rows_unit_row(in.pairs, u, i);
        const uint32_t l = rows_len_checked(in, g, st, threadIdx.x == 0u);
        uint32_t nh = 0u;
        const uint32_t nk = sc_kmers_row_long<16>(in, g, l, cand, [&](unsigned long long v) __attribute__((always_inline)) { nh += sc_probe(in.tab, in.S, in.collide, v) ? 1u : 0u; });
        const unsigned long long t = wave_sum<unsigned long long>((unsigned long long)nk | ((unsigned long long)nh << 32));
        rk[i] = (uint32_t)t; rh[i] = (uint32_t)(t >> 32); lsum += l;
    }
    if (threadIdx.x == 0u) sc_unit_out(in, u, cand, rk, rh, lsum, acc);
    rows_sums_out<1>(acc, st->c);
}
