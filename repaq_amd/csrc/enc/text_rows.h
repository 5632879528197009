// enc/text_rows.h - FASTQ text -> fixed-stride base / quality rows, read lengths, name lines + offsets (rfq_text_rows): the reverse of enc/rows_text.h
// Part of rfq_encode_kernels.h (included from there, last; not a stand-alone header).
#pragma once
// Row g is read g of the batch in interleaved order (read_loc: RFQ_PE_TWO_FILES rows 2k / 2k + 1 are record k of stream 0 / 1), its four lines are entries
// 4r .. 4r + 4 of the stream's line table (enc/index.h).  k_text_rows_sizes judges the rows from the line table alone and leaves lengths, name sizes
// (scanned to offsets by the host's scan_exclusive), maxima and sums; k_text_rows writes base and quality rows, k_text_names the name blob.  The bytes are
// the text's own: nothing is complemented, folded or dropped.
#define TR_ERR_EMPTY   (1u << 0)      // an empty line inside a row's record: the reader stops there (first_empty)
#define TR_ERR_QSHORT  (1u << 1)      // a quality line shorter than its sequence line                             (RFQ_E_UNPINNED)
#define TR_ERR_BASE    (1u << 2)      // writer, code mode: a base that is not one of A C G T N                    (RFQ_E_DATA)
// what the host reads back: zeroed per pass, first_empty = bad_row = ~0
struct TextRowsStat { uint32_t err, max_len, max_name, first_empty; unsigned long long bad_row, n_bases; };

// How a sizes kernel of 256 threads (k_text_rows_sizes, k_sel_judge) ends: every thread's longest read, longest name, bases and error bits into the verdict block
// (Stat: max_len, max_name, n_bases, err).  Wave reduce, four LDS slots, and thread 0's three atomics on the same three words - with several rows per thread, that
// many times fewer of them than with a workgroup per 256 rows - and, only where a row is at fault, one atomicOr of the error bits per wave (rare: it ends the call
// or the rows).  Every thread of the workgroup calls it; what a caller's lanes 0 wrote to LDS before the call, its thread 0 may read after it.
template <class Stat> __device__ __forceinline__ void rows_sizes_reduce(uint32_t ml, uint32_t mn, unsigned long long nb, uint32_t err, Stat* __restrict__ st) {
    __shared__ uint32_t s_ml[4], s_mn[4]; __shared__ unsigned long long s_nb[4];
    ml = wave_max(ml); mn = wave_max(mn); const uint32_t e = wave_or(err); nb = wave_sum<unsigned long long>(nb);
    if (lane_id() == 0) { s_ml[wave_id()] = ml; s_mn[wave_id()] = mn; s_nb[wave_id()] = nb; if (e) atomicOr(&st->err, e); }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = s_ml[0], b = s_mn[0]; unsigned long long c = s_nb[0];
        for (uint32_t i = 1; i < 4u; i++) { if (s_ml[i] > a) a = s_ml[i]; if (s_mn[i] > b) b = s_mn[i]; c += s_nb[i]; }
        if (a) atomicMax(&st->max_len, a);
        if (b) atomicMax(&st->max_name, b);
        if (c) atomicAdd(&st->n_bases, c);
    }
}
// grid ceil(n_rows / TS_ROWS) x 256 threads, a thread per row and TS_ITER rows per thread; the workgroup ends in rows_sizes_reduce, and an offending thread leaves
// its row with one atomicMin.  lens[g] = bases of row g, nsz[g] = bytes of its name line (64-bit: scanned in place to the offsets).
#define TS_ITER 8u
#define TS_ROWS (256u * TS_ITER)
__global__ void __launch_bounds__(256) k_text_rows_sizes(Text T, uint32_t n_rows, int32_t* __restrict__ lens, uint64_t* __restrict__ nsz, TextRowsStat* __restrict__ st) {
    uint32_t ml = 0, mn = 0, err = 0; unsigned long long nb = 0;
    for (uint32_t it = 0; it < TS_ITER; it++) {
        const uint64_t g64 = (uint64_t)blockIdx.x * TS_ROWS + it * 256u + threadIdx.x;
        if (g64 >= n_rows) break;
        const uint32_t g = (uint32_t)g64;
        int s; uint32_t r; read_loc(T, g, s, r); const uint32_t* p = t_lo(T, s) + 4 * (size_t)r;
        const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3], p4 = p[4];
        const uint32_t nl = p1 - 1 - p0, sl = p2 - 1 - p1, tl = p3 - 1 - p2, ql = p4 - 1 - p3;
        if (nl == 0 || sl == 0 || tl == 0 || ql == 0) { err |= TR_ERR_EMPTY; atomicMin(&st->first_empty, g); }
        if (ql < sl) { err |= TR_ERR_QSHORT; atomicMin(&st->bad_row, (unsigned long long)g); }
        lens[g] = (int32_t)sl; nsz[g] = nl;
        if (sl > ml) ml = sl; if (nl > mn) mn = nl; nb += sl;
    }
    rows_sizes_reduce(ml, mn, nb, err, st);
}

struct TextRowsOut {
    uint8_t* bases; uint8_t* quals;                   // [n_rows][row_len]; null = not wanted
    uint64_t row_len; uint32_t n_rows;
    uint32_t codes;                                   // bases as A0 C1 G2 T3 N4 instead of the text's bytes
    uint32_t qoff4, pad_b4, pad_q4;                   // quality offset / pad bytes, repeated in the four bytes of a word
    uint32_t vec;                                     // row_len % 16 == 0 and both row buffers 16-byte aligned: one 16-byte store per group
    uint32_t per;                                     // rows of a workgroup
};
// A C G T N -> 0 1 2 3 4 and the test in one go: bits 1-3 of the byte (A 0, C 1, T 2, G 3, N 7) index an 8-entry table whose other entries are 7; the code
// looked up in the table of ascii4_of_code (7 -> 0x00) gives the byte back exactly when it was one of the five.  bad: non-zero bytes = not A C G T N
__device__ __forceinline__ uint32_t tr_code4(uint32_t w, uint32_t& bad) {
    const uint32_t c = __builtin_amdgcn_perm(0x04070707u, 0x02030100u, (w >> 1) & 0x07070707u);
    bad |= ascii4_of_code(c) ^ w;
    return c;
}
// grid ceil(n_rows / per) x 256 threads.  The work follows the OUTPUT: a workgroup owns `per` consecutive rows, a thread one 16-byte group [k0, k0 + 16) of one
// row at a time, in GroupWalk's order (rfq_common.h).  A group that holds bases is ONE 16-byte load from the text at the text's own alignment per source - also the
// read's last, partial group wherever 16 bytes from there still lie inside the stream (what follows the line is masked off in registers); only at the very end of a
// stream is it read byte by byte.  The tail of a read and the pad are merged in registers (low_bytes) and the group is stored once (store_group16).  No LDS.
__global__ void __launch_bounds__(256) k_text_rows(Text T, TextRowsOut o, TextRowsStat* __restrict__ st) {
    const uint32_t rs = blockIdx.x * o.per;
    if (rs >= o.n_rows) return;
    const uint32_t nr = (o.n_rows - rs < o.per) ? o.n_rows - rs : o.per;
    uint32_t bad = 0; unsigned long long bad_row = ~0ull;
    for (GroupWalk w(o.row_len, 256u); w.j < nr; w.step()) {
        const uint32_t g = rs + w.j; int s; uint32_t r; read_loc(T, g, s, r);
        const uint32_t* p = t_lo(T, s) + 4 * (size_t)r;
        const uint32_t p1 = p[1], p2 = p[2], p3 = p[3], len = p2 - 1 - p1, n = t_n(T, s);
        const uint8_t* const fq = s ? T.fq[1] : T.fq[0];
        const uint64_t k0 = 16ull * w.k;
        uint32_t wb[4] = { o.pad_b4, o.pad_b4, o.pad_b4, o.pad_b4 }, wq[4] = { o.pad_q4, o.pad_q4, o.pad_q4, o.pad_q4 };
        if (k0 < len) {
            const uint32_t at = (uint32_t)k0, have = len - at < 16u ? len - at : 16u;        // bytes of the read in this group
            uint32_t b[4] = { 0, 0, 0, 0 }, q[4] = { 0, 0, 0, 0 };
            // (the quality line is at least as long as the sequence line - the sizes kernel saw to it - and lies behind it: its 16 bytes decide)
            if ((uint64_t)p3 + at + 16u <= n) {
                if (o.bases) rt_ld16(fq + p1 + at, false, b);
                if (o.quals) rt_ld16(fq + p3 + at, false, q);
            } else {
                for (uint32_t i = 0; i < have; i++) {
                    const uint32_t sh = 8u * (i & 3u);
                    if (o.bases) b[i >> 2] |= (uint32_t)fq[p1 + at + i] << sh;
                    if (o.quals) q[i >> 2] |= (uint32_t)fq[p3 + at + i] << sh;
                }
            }
            uint32_t bb = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t m = low_bytes((int)have - 4 * i);
                uint32_t x = b[i];
                if (o.codes) x = tr_code4((x & m) | (0x41414141u & ~m), bb);                     // (bytes behind the read count as 'A': never an offender)
                wb[i] = (x & m) | (o.pad_b4 & ~m);
                wq[i] = (sub_bytes(q[i], o.qoff4) & m) | (o.pad_q4 & ~m);
            }
            if (bb && o.bases) { bad |= TR_ERR_BASE; if (bad_row == ~0ull) bad_row = g; }
        }
        store_group16(o.bases, o.quals, (uint64_t)g * o.row_len + k0, o.row_len, k0, o.vec, wb, wq);
    }
    if (bad) { atomicOr(&st->err, bad); atomicMin(&st->bad_row, bad_row); }
}

// ---- a name blob: names back to back, name g's bytes wherever its source keeps them (k_text_names, k_sel_names)
#define TN_TPB 256
#define TN_TILE (TN_TPB * 16u)                // blob bytes of a workgroup: 4 KiB
// the LDS table of a tile: the names that start inside it - TN_TILE at most where every name has a byte - and one entry more, the end of the last of them (the start
// of the first name at or behind the tile's end), which closes the search from above
#define TN_RECS (TN_TILE + 1u)
// grid ceil((names_len + shift) / TN_TILE) x TN_TPB threads; src(g): the address of name g's first byte.  The work follows the BLOB: positions count from the
// 16-byte boundary at or below it (shift = blob & 15), a workgroup owns TN_TILE of them and a thread one aligned 16-byte group.  Thread 0 finds the name the tile
// starts in and the first name that starts at or behind the tile's end (binary searches in off[], the exclusive scan of the name sizes, off[n] = names_len); where
// the names in between start, relative to the tile, goes to LDS and every thread finds its group's name there.  A name may have no bytes (rfq_select_rows passes
// them through; a line of text always has one): equal offsets are searched to the LAST of them, the name that holds the byte, and a tile in which more names start
// than the LDS table holds searches off[] itself.  A group inside one name is one 16-byte load at the source's own alignment and one aligned store; a group that
// holds a boundary is put together byte by byte in registers; the blob's first and last group, where they are not whole, are stored byte by byte.
// The writer in two parts, so that a source whose names are not one run of bytes (enc/rows_tag.h: head, tag, tail) follows the same blob: name_blob_find - which
// group is this thread's, which name holds its first byte -, then the fetch of the group's bytes.
// A thread's group: blob bytes [qa, qe), stored at nb + A (nb: the 16-byte boundary at or below the blob); g: the name that holds byte qa
struct NameGroup { uint8_t* nb; uint64_t A, qa, qe; uint32_t g; };
// Every thread of the workgroup calls it (two barriers); false: the thread's group lies behind the blob.
__device__ __forceinline__ bool name_blob_find(const uint64_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ blob, uint64_t names_len, NameGroup& G) {
    __shared__ uint32_t s_rel[TN_RECS + 1]; __shared__ uint32_t s_r0, s_hi;
    const uint32_t shift = (uint32_t)((uintptr_t)blob & 15u); uint8_t* const nb = blob - shift;
    const uint64_t A0 = (uint64_t)blockIdx.x * TN_TILE;                      // (position from nb)
    const uint64_t q0 = A0 > shift ? A0 - shift : 0ull;                      // the tile's first blob byte
    if (threadIdx.x == 0) {
        uint32_t lo = 0, hi = n;                                              // off[lo] <= q0 < off[hi]
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= q0) lo = mid; else hi = mid; }
        s_r0 = lo;
        // ... and the first name that starts at or behind the tile's end (n: none does - off[n] = names_len ends the last one): the entries in between are all a
        // group of this tile can ask for (names of 53 bytes: 80 of the 4,098 entries)
        const uint64_t qt = A0 + TN_TILE - shift;
        uint32_t hi2 = n;                                                     // off[lo] < qt <= off[hi2], or hi2 = n
        while (hi2 - lo > 1) { const uint32_t mid = lo + (hi2 - lo) / 2; if (off[mid] < qt) lo = mid; else hi2 = mid; }
        s_hi = hi2;
    }
    __syncthreads();
    const uint32_t r0 = s_r0, span = s_hi - r0; const bool in_lds = span <= TN_RECS; const uint32_t cnt = in_lds ? span : 0u;
    // s_rel[k]: start of name r0 + k, in blob bytes from q0 (name r0 itself starts at or before q0: 0); beyond the tile or the names: ~0
    if (in_lds) for (uint32_t k = threadIdx.x; k <= cnt; k += TN_TPB) {
        uint32_t v = 0xFFFFFFFFu;
        if (k == 0) v = 0;
        else if ((uint64_t)r0 + k <= n) { const uint64_t d = off[r0 + k] - q0; if (d < 0xFFFFFFFFull) v = (uint32_t)d; }
        s_rel[k] = v;
    }
    __syncthreads();
    const uint64_t A = A0 + 16ull * threadIdx.x;
    if (A >= names_len + shift) return false;
    const uint64_t qa = A > shift ? A - shift : 0ull, qe = (A + 16u - shift < names_len) ? A + 16u - shift : names_len;   // this group's blob bytes [qa, qe)
    uint32_t g;
    if (in_lds) {
        const uint32_t rel = (uint32_t)(qa - q0);
        uint32_t lo = 0, hi = cnt;                                            // s_rel[lo] <= rel < s_rel[hi]: name r0 + cnt starts at or behind the tile's end
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (s_rel[mid] <= rel) lo = mid; else hi = mid; }
        g = r0 + lo;
    } else {
        uint32_t lo = r0, hi = s_hi;                                          // off[lo] <= qa < off[hi] (hi = n: off[n] = names_len)
        while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (off[mid] <= qa) lo = mid; else hi = mid; }
        g = lo;
    }
    G.nb = nb; G.A = A; G.qa = qa; G.qe = qe; G.g = g;
    return true;
}
// a group put together in registers (h0: bytes 0 .. 7, h1: 8 .. 15): one aligned store where it is whole, else - the blob's first or last group - byte by byte
__device__ __forceinline__ void name_group_store(const NameGroup& G, uint8_t* __restrict__ blob, unsigned long long h0, unsigned long long h1) {
    const uint32_t nby = (uint32_t)(G.qe - G.qa);
    if (G.qe - G.qa == 16u) *(uint4*)(G.nb + G.A) = make_uint4((uint32_t)h0, (uint32_t)(h0 >> 32), (uint32_t)h1, (uint32_t)(h1 >> 32));
    else for (uint32_t i = 0; i < nby; i++) blob[G.qa + i] = (uint8_t)(i < 8u ? h0 >> (8u * i) : h1 >> (8u * (i - 8u)));
}
template <class Src> __device__ __forceinline__ void name_blob_write(const Src& src, const uint64_t* __restrict__ off, uint32_t n, uint8_t* __restrict__ blob, uint64_t names_len) {
    NameGroup G;
    if (!name_blob_find(off, n, blob, names_len, G)) return;
    uint8_t* const nb = G.nb; const uint64_t A = G.A, qa = G.qa, qe = G.qe; uint32_t g = G.g;
    uint64_t beg = off[g], end = off[g + 1];
    const bool whole = qe - qa == 16u;
    if (whole && qe <= end) {
        uint32_t w[4]; rt_ld16(src(g) + (qa - beg), false, w);
        *(uint4*)(nb + A) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    unsigned long long h0 = 0, h1 = 0; const uint32_t nby = (uint32_t)(qe - qa);
    const uint8_t* p = src(g);
    for (uint32_t i = 0; i < nby; i++) {
        const uint64_t q = qa + i;
        while (q >= end) { g++; beg = end; end = off[g + 1]; p = src(g); }
        const unsigned long long c = p[q - beg];
        if (i < 8u) h0 |= c << (8u * i); else h1 |= c << (8u * (i - 8u));
    }
    name_group_store(G, blob, h0, h1);
}

// ---- names: the first line of every row, back to back (name_blob_write over the rows' name lines)
struct TextNameSrc {
    const Text& T;
    __device__ __forceinline__ const uint8_t* operator()(uint32_t g) const { int s; uint32_t r; read_loc(T, g, s, r); return (s ? T.fq[1] : T.fq[0]) + t_lo(T, s)[4 * (size_t)r]; }
};
__global__ void __launch_bounds__(TN_TPB) k_text_names(Text T, const uint64_t* __restrict__ off, uint32_t n_rows, uint8_t* __restrict__ blob, uint64_t names_len) {
    name_blob_write(TextNameSrc{ T }, off, n_rows, blob, names_len);
}
