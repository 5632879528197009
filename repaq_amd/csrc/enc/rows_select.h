// enc/rows_select.h - rows -> the kept rows, trimmed to a window each, with their lengths, names and name offsets (rfq_select_rows): the step between
// rfq_decode_rows / rfq_text_rows and rfq_encode_rows / rfq_rows_to_text
// Part of rfq_encode_kernels.h (included from there, last; not a stand-alone header).  The pieces of a compacting call that rfq_merge_rows (enc/rows_merge.h) takes
// from here as they are: the table entry (SelRow), the tables body (rows_tables), the row writers' arguments (RowsOut) and the names kernel (k_sel_names).
#pragma once
// k_sel_judge resolves every row's window, validates it and decides who stays (mask, min_len, the pair rule); it leaves a kept flag and the kept name size per
// row (scanned by the host's scan_exclusive to the output row index and the output name offset), the maxima, sums and drop counts.  After ONE read-back the host
// decides; k_sel_tables then turns the two scans into tables per OUTPUT row (source row, window, name offset), which the two writers follow: k_sel_rows the base
// and quality rows, k_sel_names the name blob.  The bytes are the rows' own: nothing is transformed.
#define SL_ERR_LEN     (1u << 0)      // a length that is negative or greater than the input row_len                (RFQ_E_ARG; all three)
#define SL_ERR_WIN     (1u << 1)      // a window that starts below 0, has a negative length or ends behind the read
#define SL_ERR_NOFF    (1u << 2)      // name offsets that decrease, or a last one past names_len
struct SelIn {
    const int32_t* lens; const uint64_t* name_off;                            // [n_rows], [n_rows + 1] or null: rows without names
    const uint8_t* keep; const int32_t* start; const int32_t* len;            // [n_rows] each, or null: every row / 0 / to the end of the read
    uint64_t names_len;
    uint32_t n_rows, row_len;                                                 // (row_len: the input stride)
    uint32_t pairs, min_len;
};
// what the host reads back: zeroed per call, bad_row = ~0
struct SelStat { uint32_t err, max_len, max_name, pad; unsigned long long bad_row, n_bases, d_mask, d_short, d_mate; };
// one entry per OUTPUT row: where it comes from
struct SelRow { uint32_t src, start, len, pad; };

// The window of row i, and whether the row stands on its own: 0 it does, 1 its mask byte is 0, 2 its window is shorter than min_len.  err: what is wrong with the
// row's length or window (its window then counts as empty; the call is refused anyway).  start + len is formed in 64 bits.
__device__ __forceinline__ uint32_t sel_window(const SelIn& in, uint32_t i, uint32_t& start, uint32_t& len, uint32_t& err) {
    const int32_t l = in.lens[i];
    const long long s = in.start ? (long long)in.start[i] : 0ll;
    const long long w = in.len ? (long long)in.len[i] : (long long)l - s;
    err = 0;
    if (l < 0 || (uint32_t)l > in.row_len) err = SL_ERR_LEN;
    else if (s < 0 || w < 0 || s + w > (long long)l) err = SL_ERR_WIN;
    start = err ? 0u : (uint32_t)s; len = err ? 0u : (uint32_t)w;
    if (in.keep && !in.keep[i]) return 1u;
    return len < in.min_len ? 2u : 0u;
}

// grid ceil(n_rows / SJ_ROWS) x 256 threads, a thread per row and SJ_ITER rows per thread; the workgroup ends in rows_sizes_reduce (enc/text_rows.h) with the three
// drop counts beside it: the same barrier, three more atomics of thread 0.  The mate of row g is row g ^ 1: its mask byte and window are read again rather than
// shuffled (the same cache lines; no rendezvous inside the loop a short last workgroup leaves early).  flag[g] = 1 for a kept row, nsz[g] = bytes of its name (0
// for a dropped row; 64-bit: scanned in place to the output offsets; null for rows without names).  All rows are judged, kept or not; an offending thread leaves
// its row with one atomicMin.
#define SJ_ITER 8u
#define SJ_ROWS (256u * SJ_ITER)
// The body is a template over a Rule, so that a call with a further rule per unit (rfq_group_rows, enc/rows_group.h) judges through the same lines: rule.drops(g, err)
// - the rule of its own by which row g falls, asked of every row the mask lets through, in front of `short` (and what is wrong with the row's input to it);
// rule.bad(st, g) - where an offending row is left; rule.row(g, kept, nl) - the verdict of row g and the bytes of its name; rule.finish(st, dr) - what the rule itself
// sums up (dr: the thread's rows that fell by it), called by every thread behind the common reduction.
// A rule whose kept names GROW (enc/rows_tag.h: a tag is written into them) says so here and has rule.grow(g, e, re): the bytes row g's name gains if it is kept
// (e: what is wrong with the row's length or window, re: what is wrong with the rule's own input).  The other rules do not have the member and keep their code.
template <class Rule> struct sel_rule_grows { static constexpr bool value = false; };
template <class Stat, class Rule> __device__ __forceinline__ void sel_judge(const SelIn& in, Stat* __restrict__ st, Rule& rule) {
    __shared__ uint32_t s_dm[4], s_ds[4], s_dt[4];
    uint32_t ml = 0, mn = 0, err = 0, dm = 0, ds = 0, dt = 0, dr = 0; unsigned long long nb = 0;
    for (uint32_t it = 0; it < SJ_ITER; it++) {
        const uint64_t g64 = (uint64_t)blockIdx.x * SJ_ROWS + it * 256u + threadIdx.x;
        if (g64 >= in.n_rows) break;
        const uint32_t g = (uint32_t)g64;
        uint32_t s0, w, e; uint32_t why = sel_window(in, g, s0, w, e);
        uint64_t nl = 0;
        if (in.name_off) {
            const uint64_t a = in.name_off[g], b = in.name_off[g + 1];
            if (b < a || (g + 1u == in.n_rows && b > in.names_len)) e |= SL_ERR_NOFF; else nl = b - a;
        }
        uint32_t re = 0; const bool falls = rule.drops(g, re);
        if constexpr (sel_rule_grows<Rule>::value) nl += rule.grow(g, e, re);
        if (why != 1u && falls) why = 4u;                                    // (counted behind the mask and in front of `short`)
        if (why == 0 && in.pairs) { uint32_t ms, mw, me; if (sel_window(in, g ^ 1u, ms, mw, me) != 0) why = 3u; }      // (n_rows is even: the host saw to it)
        if (e) { err |= e; atomicMin(&st->bad_row, (unsigned long long)g); }
        if (re) { err |= re; rule.bad(st, g); }
        const bool kept = why == 0;
        rule.row(g, kept, nl);
        dm += why == 1u; ds += why == 2u; dt += why == 3u; dr += why == 4u;
        if (kept) {
            const uint32_t n32 = nl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nl;
            if (w > ml) ml = w; if (n32 > mn) mn = n32; nb += w;
        }
    }
    dm = wave_sum(dm); ds = wave_sum(ds); dt = wave_sum(dt);
    if (lane_id() == 0) { const int w = wave_id(); s_dm[w] = dm; s_ds[w] = ds; s_dt[w] = dt; }
    rows_sizes_reduce(ml, mn, nb, err, st);                                  // (its barrier stands between the three stores above and thread 0's loads below)
    if (threadIdx.x == 0) {
        unsigned long long x = s_dm[0], y = s_ds[0], z = s_dt[0];
        for (uint32_t i = 1; i < 4u; i++) { x += s_dm[i]; y += s_ds[i]; z += s_dt[i]; }
        if (x) atomicAdd(&st->d_mask, x);
        if (y) atomicAdd(&st->d_short, y);
        if (z) atomicAdd(&st->d_mate, z);
    }
    rule.finish(st, dr);
}
// rfq_select_rows: no further rule; the verdict goes to flag[] / nsz[]
struct SelPlain {
    uint32_t* __restrict__ flag; uint64_t* __restrict__ nsz;
    __device__ __forceinline__ bool drops(uint32_t, uint32_t&) const { return false; }
    __device__ __forceinline__ void bad(SelStat*, uint32_t) const {}
    __device__ __forceinline__ void row(uint32_t g, bool kept, uint64_t nl) const { flag[g] = kept ? 1u : 0u; if (nsz) nsz[g] = kept ? nl : 0ull; }
    __device__ __forceinline__ void finish(SelStat*, uint32_t) const {}
};
__global__ void __launch_bounds__(256) k_sel_judge(SelIn in, uint32_t* __restrict__ flag, uint64_t* __restrict__ nsz, SelStat* __restrict__ st) {
    SelPlain rule{ flag, nsz };
    sel_judge(in, st, rule);
}

// The tables of a compacting call, a thread per INPUT unit (select: a row, merge: a pair): pos[] / noff[] are the exclusive scans of the kept flags / kept name sizes
// with their totals behind them (pos[n] = n_out), so unit i was kept exactly when pos[i + 1] != pos[i], and is output row pos[i].  entry(i, len) yields the SelRow of
// a kept unit as a uint4 and the output row's length.  tab / ooff: the context's tables the writers search; d_lens / d_name_off: the caller's, where asked for (the
// same values: no copy behind this).  noff null: rows without names.
template <class Entry> __device__ __forceinline__ void rows_tables(const Entry& entry, uint32_t n, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ noff,
        SelRow* __restrict__ tab, uint64_t* __restrict__ ooff, int32_t* __restrict__ d_lens, uint64_t* __restrict__ d_name_off) {
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64, j = pos[i];
    if (i == 0 && noff) { const uint32_t n_out = pos[n]; const uint64_t t = noff[n]; ooff[n_out] = t; if (d_name_off) d_name_off[n_out] = t; }
    if (pos[i + 1] == j) return;
    int32_t len; const uint4 e = entry(i, len);
    *(uint4*)(tab + j) = e;
    if (d_lens) d_lens[j] = len;
    if (noff) { const uint64_t t = noff[i]; ooff[j] = t; if (d_name_off) d_name_off[j] = t; }
}
// grid ceil(n_rows / 256) x 256 threads: the entry of a kept row is (the row, its window's start, its window's length, 0)
struct SelEntry {
    const SelIn& in;
    __device__ __forceinline__ uint4 operator()(uint32_t i, int32_t& len) const { uint32_t s0, w, e; (void)sel_window(in, i, s0, w, e); len = (int32_t)w; return make_uint4(i, s0, w, 0u); }
};
__global__ void __launch_bounds__(256) k_sel_tables(SelIn in, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ noff, SelRow* __restrict__ tab,
                                                    uint64_t* __restrict__ ooff, int32_t* __restrict__ d_lens, uint64_t* __restrict__ d_name_off) {
    rows_tables(SelEntry{ in }, in.n_rows, pos, noff, tab, ooff, d_lens, d_name_off);
}

// what a row writer of a compacting call takes (k_sel_rows; k_merge_rows and k_merge_rows_any of enc/rows_merge.h)
struct RowsOut {
    const uint8_t* sb; const uint8_t* sq;             // the input rows [n_in][row_len_in]; select: null with its output; merge: both, whichever output is wanted
    uint8_t* bases; uint8_t* quals;                   // [n_out][row_len]; null = not wanted
    uint64_t row_len_in, total_in;                    // input stride; bytes of an input row buffer (n_in * row_len_in)
    uint64_t row_len; uint32_t n_out;
    uint32_t pad_b4, pad_q4;                          // pad bytes, repeated in the four bytes of a word
    uint32_t vec_in;                                  // row_len_in % 16 == 0 and the input buffers that are read 16-byte aligned: the aligned groups of a row may be loaded whole
    uint32_t vec;                                     // row_len % 16 == 0 and both output buffers 16-byte aligned: one 16-byte store per group
    uint32_t per;                                     // output rows of a workgroup
    uint32_t ascii;                                   // merge: the bases are letters, not codes (select leaves it 0 and never reads it)
};
// grid ceil(n_out / per) x 256 threads.  The work follows the OUTPUT: a workgroup owns `per` consecutive output rows, a thread one 16-byte group [k0, k0 + 16) of
// one row at a time, in GroupWalk's order (rfq_common.h).  A group that holds bases is ONE load of 16 source bytes at
// the source's own alignment (the window start makes most of them unaligned also for aligned rows): from the one or two aligned groups of the source row that hold
// them where both lie inside that row (rt_ld16's groups form), else one 16-byte load wherever 16 bytes from there still lie inside the input buffer; only behind that,
// at the very end of the buffer, byte by byte.  What lies behind the window is masked off in registers and replaced by the pad (low_bytes), and the group is stored
// once (store_group16).  No LDS.
__global__ void __launch_bounds__(256) k_sel_rows(RowsOut o, const SelRow* __restrict__ tab) {
    const uint32_t rs = blockIdx.x * o.per;
    if (rs >= o.n_out) return;
    const uint32_t nr = (o.n_out - rs < o.per) ? o.n_out - rs : o.per;
    for (GroupWalk w(o.row_len, 256u); w.j < nr; w.step()) {
        const uint32_t g = rs + w.j;
        const uint4 t = *(const uint4*)(tab + g);                            // (source row, window start, window length)
        const uint32_t len = t.z;
        const uint64_t k0 = 16ull * w.k;
        uint32_t wb[4] = { o.pad_b4, o.pad_b4, o.pad_b4, o.pad_b4 }, wq[4] = { o.pad_q4, o.pad_q4, o.pad_q4, o.pad_q4 };
        if (k0 < len) {
            const uint32_t at = (uint32_t)k0, have = len - at < 16u ? len - at : 16u;        // bytes of the window in this group
            const uint64_t oin = (uint64_t)t.y + at, p = (uint64_t)t.x * o.row_len_in + oin;   // where they start: in the source row, in the input buffer
            uint32_t b[4] = { 0, 0, 0, 0 }, q[4] = { 0, 0, 0, 0 };
            if (o.vec_in && (oin & ~15ull) + ((oin & 15u) ? 32u : 16u) <= o.row_len_in) {
                if (o.bases) rt_ld16(o.sb + p, true, b);
                if (o.quals) rt_ld16(o.sq + p, true, q);
            } else if (p + 16u <= o.total_in) {
                if (o.bases) rt_ld16(o.sb + p, false, b);
                if (o.quals) rt_ld16(o.sq + p, false, q);
            } else {
                for (uint32_t i = 0; i < have; i++) {
                    const uint32_t sh = 8u * (i & 3u);
                    if (o.bases) b[i >> 2] |= (uint32_t)o.sb[p + i] << sh;
                    if (o.quals) q[i >> 2] |= (uint32_t)o.sq[p + i] << sh;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t m = low_bytes((int)have - 4 * i);
                wb[i] = (b[i] & m) | (o.pad_b4 & ~m);
                wq[i] = (q[i] & m) | (o.pad_q4 & ~m);
            }
        }
        store_group16(o.bases, o.quals, (uint64_t)g * o.row_len + k0, o.row_len, k0, o.vec, wb, wq);
    }
}

// ---- names: the whole name of every kept row, back to back (name_blob_write, enc/text_rows.h, over the OUTPUT blob: off[] are the output offsets, off[n_out] =
// names_len).  Output name g is input name tab[g].src: its bytes start at names + in_off[tab[g].src].  A name may have no bytes here (the encoder refuses it later,
// this call does not).
struct SelNameSrc {
    const uint8_t* names; const uint64_t* in_off; const SelRow* tab;
    __device__ __forceinline__ const uint8_t* operator()(uint32_t g) const { return names + in_off[tab[g].src]; }
};
__global__ void __launch_bounds__(TN_TPB) k_sel_names(const uint8_t* __restrict__ names, const uint64_t* __restrict__ in_off, const SelRow* __restrict__ tab,
                                                      const uint64_t* __restrict__ off, uint32_t n_out, uint8_t* __restrict__ blob, uint64_t names_len) {
    name_blob_write(SelNameSrc{ names, in_off, tab }, off, n_out, blob, names_len);
}
