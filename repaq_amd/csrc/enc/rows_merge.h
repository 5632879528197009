// enc/rows_merge.h - pairs of rows -> one row per overlapping pair: the fragment both mates were read from, `insert` bases long, the consensus of the two where they
// overlap, under R1's name (rfq_merge_rows): what consumes the insert sizes rfq_adapter_rows leaves.  It moves bytes and decides nothing about the alignment.
// Part of rfq_encode_kernels.h (included from there, last: it uses rows_select.h's table entry, tables body (rows_tables), writers' arguments (RowsOut) and names
// kernel, rows_lanes.h's 16-byte pieces and rows_adapter.h's base classes; not a stand-alone header).
#pragma once
// The shape is rfq_select_rows': k_merge_judge validates EVERY pair and leaves a merged flag and the merged name size per pair (scanned by the host's scan_exclusive
// to the output row index and the output name offset) with the maxima and sums; after ONE read-back the host decides; k_merge_tables turns the two scans into a table
// per OUTPUT row, which the two writers follow: k_merge_rows (or k_merge_rows_any) the base and quality rows, k_sel_names - as it is - the name blob.
// Fragment coordinates p in [0, ins): R1 covers p < min(l1, ins) with its own bytes, R2 covers p >= ins - l2 with (comp(r2[i]), q2[i]), i = ins - 1 - p (include/rfq_hip.h
// has the rule for a position both cover).
#define MG_ERR_LEN     0u             // a length that is negative or greater than the input row_len                (RFQ_E_ARG; all three)
#define MG_ERR_INS     1u             // a pair with insert >= 0 and no position that both mates cover
#define MG_ERR_NOFF    2u             // name offsets that decrease, or a last one past names_len
struct MergeIn {
    const int32_t* lens; const int32_t* insert; const uint64_t* name_off;     // [n_rows], [n_rows / 2], [n_rows + 1] or null: rows without names
    uint64_t names_len;
    uint32_t n_rows, n_pairs, row_len;                                        // (row_len: the input stride)
};
// what the host reads back: zeroed per call, bad_row = ~0.  bad_row is a KEY: (row << 2) | MG_ERR_* of the first offender (a pair counts as its row 2k), so that the
// one atomicMin also says which rule the first offender broke.
struct MergeStat { uint32_t err, max_len, max_name, pad; unsigned long long bad_row, n_bases, overlap; };

// The pair k as the judge and the tables kernel see it: its lengths (0 for a bad one), its insert, and what is wrong with it as bits 1 << MG_ERR_* (bad: the key of
// its first offender, or ~0).  merged: insert >= 0 and nothing wrong.
struct MgPair { uint32_t l1, l2; int32_t ins; uint32_t err; unsigned long long bad; bool merged; };
__device__ __forceinline__ MgPair mg_pair(const MergeIn& in, uint32_t k) {
    MgPair r; const int32_t a = in.lens[2u * k], b = in.lens[2u * k + 1u];
    r.ins = in.insert[k]; r.err = 0u; r.bad = ~0ull;
    const bool bad1 = a < 0 || (uint32_t)a > in.row_len, bad2 = b < 0 || (uint32_t)b > in.row_len;
    r.l1 = bad1 ? 0u : (uint32_t)a; r.l2 = bad2 ? 0u : (uint32_t)b;
    if (bad1 || bad2) { r.err = 1u << MG_ERR_LEN; r.bad = ((unsigned long long)(2u * k + (bad1 ? 0u : 1u)) << 2) | MG_ERR_LEN; }
    else if (r.ins >= 0 && (r.l1 == 0u || r.l2 == 0u || r.ins == 0 || (uint32_t)r.ins > r.l1 + r.l2 - 1u)) {
        r.err = 1u << MG_ERR_INS; r.bad = ((unsigned long long)(2u * k) << 2) | MG_ERR_INS;
    }
    r.merged = r.ins >= 0 && r.err == 0u;
    return r;
}

// grid ceil(n_pairs / MJ_PAIRS) x 256 threads, a thread per pair and MJ_ITER pairs per thread; the workgroup ends in rows_sizes_reduce (enc/text_rows.h) with the
// overlap sum beside it: the same barrier, one more atomic of thread 0.  flag[k] = 1 for a merged pair, nsz[k] = bytes of R1's name (0 for a pair that is not merged;
// 64-bit: scanned in place to the output offsets; null for rows without names).  All pairs are judged, merged or not - both rows' lengths and both rows' name offsets;
// an offending thread leaves its key with one atomicMin.
#define MJ_ITER 8u
#define MJ_PAIRS (256u * MJ_ITER)
__global__ void __launch_bounds__(256) k_merge_judge(MergeIn in, uint32_t* __restrict__ flag, uint64_t* __restrict__ nsz, MergeStat* __restrict__ st) {
    __shared__ unsigned long long s_ov[4];
    uint32_t ml = 0, mn = 0, err = 0; unsigned long long nb = 0, ov = 0;
    for (uint32_t it = 0; it < MJ_ITER; it++) {
        const uint64_t k64 = (uint64_t)blockIdx.x * MJ_PAIRS + it * 256u + threadIdx.x;
        if (k64 >= in.n_pairs) break;
        const uint32_t k = (uint32_t)k64;
        MgPair p = mg_pair(in, k);
        uint64_t nl = 0;
        if (in.name_off) {
            const uint64_t a = in.name_off[2u * k], b = in.name_off[2u * k + 1u], c = in.name_off[2u * k + 2u];
            const uint32_t first = b < a ? 0u : 1u;                          // (the row whose offsets are at fault, if one is)
            if (b < a || c < b || (k + 1u == in.n_pairs && c > in.names_len)) {
                const unsigned long long key = ((unsigned long long)(2u * k + first) << 2) | MG_ERR_NOFF;
                p.err |= 1u << MG_ERR_NOFF; if (key < p.bad) p.bad = key;
                p.merged = false;
            } else nl = b - a;
        }
        if (p.err) { err |= p.err; atomicMin(&st->bad_row, p.bad); }
        flag[k] = p.merged ? 1u : 0u;
        if (nsz) nsz[k] = p.merged ? nl : 0ull;
        if (p.merged) {
            const uint32_t ins = (uint32_t)p.ins, n32 = nl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nl;
            if (ins > ml) ml = ins; if (n32 > mn) mn = n32; nb += ins;
            ov += (p.l1 < ins ? p.l1 : ins) - (ins > p.l2 ? ins - p.l2 : 0u);    // positions [max(0, ins - l2), min(l1, ins)): at least one
        }
    }
    ov = wave_sum<unsigned long long>(ov);
    if (lane_id() == 0) s_ov[wave_id()] = ov;
    rows_sizes_reduce(ml, mn, nb, err, st);                                  // (its barrier stands between the store above and thread 0's loads below)
    if (threadIdx.x == 0) { const unsigned long long x = s_ov[0] + s_ov[1] + s_ov[2] + s_ov[3]; if (x) atomicAdd(&st->overlap, x); }
}

// grid ceil(n_pairs / 256) x 256 threads, a thread per INPUT pair: rows_tables (enc/rows_select.h) over pairs.  The entry of output row j is a SelRow read as
// (src = row 2k, start = l1, len = ins, pad = l2): src stands where k_sel_names reads it.
struct MergeEntry {
    const MergeIn& in;
    __device__ __forceinline__ uint4 operator()(uint32_t k, int32_t& len) const { const MgPair p = mg_pair(in, k); len = p.ins; return make_uint4(2u * k, p.l1, (uint32_t)p.ins, p.l2); }
};
__global__ void __launch_bounds__(256) k_merge_tables(MergeIn in, const uint32_t* __restrict__ pos, const uint64_t* __restrict__ noff, SelRow* __restrict__ tab,
                                                      uint64_t* __restrict__ ooff, int32_t* __restrict__ d_lens, uint64_t* __restrict__ d_name_off) {
    rows_tables(MergeEntry{ in }, in.n_pairs, pos, noff, tab, ooff, d_lens, d_name_off);
}

// ---- four bytes at a time
// 0xFF in every byte of w that is one of A C G T (code mode: below 4; ASCII mode: the letter in either case)
__device__ __forceinline__ uint32_t mg_acgt(uint32_t ascii, uint32_t w) {
    if (!ascii) return ((~rows_ge(w, 4u) & 0x80808080u) >> 7) * 0xFFu;
    const uint32_t f = w & 0xDFDFDFDFu;
    return eq_bytes_full(f, 0x41414141u) | eq_bytes_full(f, 0x43434343u) | eq_bytes_full(f, 0x47474747u) | eq_bytes_full(f, 0x54545454u);
}
// rfq_adapter_rows' complement as a byte map: codes 0 <-> 3 and 1 <-> 2 (an XOR with 3 below 4), letters A <-> T (0x41 ^ 0x54 = 0x15) and C <-> G (0x43 ^ 0x47 = 0x04)
// in the case they have; every other byte is itself
__device__ __forceinline__ uint32_t mg_comp(uint32_t ascii, uint32_t w) {
    if (!ascii) return w ^ (mg_acgt(0u, w) & 0x03030303u);
    const uint32_t f = w & 0xDFDFDFDFu;
    return w ^ ((eq_bytes_full(f, 0x41414141u) | eq_bytes_full(f, 0x54545454u)) & 0x15151515u) ^ ((eq_bytes_full(f, 0x43434343u) | eq_bytes_full(f, 0x47474747u)) & 0x04040404u);
}
// 0xFF in every byte where x >= y (bytes are unsigned): the low seven bits by a subtraction that cannot borrow across bytes, the top bits beside it
__device__ __forceinline__ uint32_t mg_ge(uint32_t x, uint32_t y) {
    const uint32_t t = (x | 0x80808080u) - (y & 0x7F7F7F7Fu);
    return ((((x & ~y) | (~(x ^ y) & t)) & 0x80808080u) >> 7) * 0xFFu;
}
// the four bytes of a word in reverse order: one v_perm_b32
__device__ __forceinline__ uint32_t mg_rev4(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x00010203u); }
// The rule for four positions.  (b1, q1): R1's bytes, (b2, q2): R2's, reversed and complemented; m1 / m2: 0xFF in the bytes R1 / R2 covers.  Bytes neither covers
// come back 0.
__device__ __forceinline__ void mg_consensus(uint32_t ascii, uint32_t b1, uint32_t q1, uint32_t b2, uint32_t q2, uint32_t m1, uint32_t m2, uint32_t& ob, uint32_t& oq) {
    const uint32_t a1 = mg_acgt(ascii, b1), a2 = mg_acgt(ascii, b2), fold = ascii ? 0xDFDFDFDFu : 0xFFFFFFFFu;
    const uint32_t agree = eq_bytes_full(b1 & fold, b2 & fold) & a1;         // (equal to a base of R1's: R2's is one as well)
    const uint32_t only1 = a1 & ~a2, only2 = a2 & ~a1, rest = ~(agree | only1 | only2);
    const uint32_t ge = mg_ge(q1, q2), hi = (q1 & ge) | (q2 & ~ge), lo = (q2 & ge) | (q1 & ~ge);
    const uint32_t both = m1 & m2;
    const uint32_t take1 = (m1 & ~m2) | (both & (agree | only1 | (rest & ge)));
    ob = (b1 & take1) | (b2 & m2 & ~take1);
    const uint32_t s1 = (m1 & ~m2) | (both & only1), s2 = (m2 & ~m1) | (both & only2);
    oq = (q1 & s1) | (q2 & s2) | (hi & both & agree) | (sub_bytes(hi, lo) & both & rest);
}

// 16 bytes of buf that END in front of byte `end` of the row that starts at rowbase, in reverse order: w holds source bytes end - 1, end - 2, ..., end - 16.  Only
// bytes j in [f, t) of w are wanted (source bytes end - 1 - j: the caller sees to it that they lie inside the row); the others come back as whatever the load found
// inside the buffer, or 0.  One 16-byte load at the bytes' own alignment wherever all 16 lie inside the buffer, byte by byte only at the buffer's two ends.
__device__ __forceinline__ void mg_ld16_rev(const uint8_t* buf, uint64_t total, uint64_t rowbase, uint32_t end, uint32_t f, uint32_t t, uint32_t (&w)[4]) {
    const long long p = (long long)rowbase + (long long)end - 16ll;
    if (p >= 0 && (unsigned long long)p + 16ull <= total) {
        uint32_t x[4]; rt_ld16(buf + p, false, x);
        w[0] = mg_rev4(x[3]); w[1] = mg_rev4(x[2]); w[2] = mg_rev4(x[1]); w[3] = mg_rev4(x[0]);
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
        for (uint32_t j = f; j < t; j++) w[j >> 2] |= (uint32_t)buf[rowbase + (end - 1u - j)] << (8u * (j & 3u));
    }
}
// grid ceil(n_out / per) x 256 threads.  The work follows the OUTPUT, as in k_sel_rows: a workgroup owns `per` consecutive merged rows, a thread one 16-byte group
// [k0, k0 + 16) of one row at a time, in GroupWalk's order (rfq_common.h).  R1's part of the group is rows_ld16 at offset k0 of row 2k (the window starts at 0: with
// aligned rows the aligned load).  R2's part is source bytes [ins - 16 - k0, ins - k0) of row 2k + 1: one load at their own alignment (mg_ld16_rev), reversed in
// registers (the four words swapped, v_perm_b32 in each) and complemented by SWAR; the quality group takes the same load and the same reversal.  The rule is byte
// masks and selects (mg_consensus); what lies behind the read is the pad (low_bytes), and the group is stored once (store_group16).  No LDS, no atomics.
__global__ void __launch_bounds__(256) k_merge_rows(RowsOut o, const SelRow* __restrict__ tab) {
    const uint32_t rs = blockIdx.x * o.per;
    if (rs >= o.n_out) return;
    const uint32_t nr = (o.n_out - rs < o.per) ? o.n_out - rs : o.per;
    for (GroupWalk w(o.row_len, 256u); w.j < nr; w.step()) {
        const uint32_t g = rs + w.j;
        const uint4 t = *(const uint4*)(tab + g);                            // (row 2k, l1, ins, l2)
        const uint32_t l1 = t.y, ins = t.z, l2 = t.w;
        const uint64_t k0 = 16ull * w.k;
        uint32_t wb[4] = { o.pad_b4, o.pad_b4, o.pad_b4, o.pad_b4 }, wq[4] = { o.pad_q4, o.pad_q4, o.pad_q4, o.pad_q4 };
        if (k0 < ins) {
            const uint32_t at = (uint32_t)k0, have = ins - at < 16u ? ins - at : 16u;        // positions of the fragment in this group
            const uint32_t c1 = l1 < ins ? l1 : ins, s2 = ins > l2 ? ins - l2 : 0u;          // R1 covers [0, c1), R2 [s2, ins)
            const uint32_t n1 = c1 > at ? (c1 - at < 16u ? c1 - at : 16u) : 0u;               // bytes [0, n1) of the group are R1's,
            const uint32_t f2 = s2 > at ? (s2 - at < 16u ? s2 - at : 16u) : 0u;               // bytes [f2, have) R2's
            const uint64_t base1 = (uint64_t)t.x * o.row_len_in, base2 = base1 + o.row_len_in;
            uint32_t b1[4] = { 0, 0, 0, 0 }, q1[4] = { 0, 0, 0, 0 }, b2[4] = { 0, 0, 0, 0 }, q2[4] = { 0, 0, 0, 0 };
            if (n1) { rows_ld16(o.sb, o.vec_in, o.total_in, base1, at, c1, b1); rows_ld16(o.sq, o.vec_in, o.total_in, base1, at, c1, q1); }
            if (f2 < have) { mg_ld16_rev(o.sb, o.total_in, base2, ins - at, f2, have, b2); mg_ld16_rev(o.sq, o.total_in, base2, ins - at, f2, have, q2); }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t mh = low_bytes((int)have - 4 * i), m1 = low_bytes((int)n1 - 4 * i), m2 = mh & ~low_bytes((int)f2 - 4 * i);
                uint32_t ob, oq; mg_consensus(o.ascii, b1[i], q1[i], mg_comp(o.ascii, b2[i]), q2[i], m1, m2, ob, oq);
                wb[i] = (ob & mh) | (o.pad_b4 & ~mh);
                wq[i] = (oq & mh) | (o.pad_q4 & ~mh);
            }
        }
        store_group16(o.bases, o.quals, (uint64_t)g * o.row_len + k0, o.row_len, k0, o.vec, wb, wq);
    }
}

// ---- the second formulation (RFQ_MERGE=general): a lane per output byte, the rule as it is written in include/rfq_hip.h
__device__ __forceinline__ uint8_t mg_comp_byte(uint32_t ascii, uint8_t c) {
    if (!ascii) return c < 4u ? (uint8_t)(3u - c) : c;
    switch (c) { case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; case 'a': return 't'; case 't': return 'a'; case 'c': return 'g'; case 'g': return 'c';
    default: return c; }
}
// grid ceil(n_out * row_len / 256) x 256 threads: thread t writes byte t % row_len of output row t / row_len, in each buffer that is wanted.  Only bytes in front of
// a read's length are read, so never a byte outside the rows.
__global__ void __launch_bounds__(256) k_merge_rows_any(RowsOut o, const SelRow* __restrict__ tab) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)o.n_out * o.row_len) return;
    const uint64_t g = t / o.row_len, p = t % o.row_len;
    const SelRow r = tab[g];
    const uint32_t l1 = r.start, ins = r.len, l2 = r.pad;
    uint8_t b = (uint8_t)o.pad_b4, q = (uint8_t)o.pad_q4;
    if (p < ins) {
        const bool c1 = p < l1, c2 = p + l2 >= ins;
        const uint64_t at1 = (uint64_t)r.src * o.row_len_in + p, at2 = ((uint64_t)r.src + 1u) * o.row_len_in + (ins - 1u - p);
        const uint8_t x1 = c1 ? o.sb[at1] : (uint8_t)0, y1 = c1 ? o.sq[at1] : (uint8_t)0;
        const uint8_t x2 = c2 ? mg_comp_byte(o.ascii, o.sb[at2]) : (uint8_t)0, y2 = c2 ? o.sq[at2] : (uint8_t)0;
        if (c1 && c2) {
            const uint32_t k1 = ar_cls(o.ascii, x1), k2 = ar_cls(o.ascii, x2);
            if (k1 < 4u && k1 == k2) { b = x1; q = y1 > y2 ? y1 : y2; }
            else if (k1 < 4u && k2 >= 4u) { b = x1; q = y1; }
            else if (k2 < 4u && k1 >= 4u) { b = x2; q = y2; }
            else if (y1 >= y2) { b = x1; q = (uint8_t)(y1 - y2); }
            else { b = x2; q = (uint8_t)(y2 - y1); }
        } else if (c1) { b = x1; q = y1; }
        else { b = x2; q = y2; }
    }
    if (o.bases) o.bases[t] = b;
    if (o.quals) o.quals[t] = q;
}
