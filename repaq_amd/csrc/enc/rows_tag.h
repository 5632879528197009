// enc/rows_tag.h - a tag of the read's own bases written into the kept names while rfq_select_rows writes the name blob (rfq_name_tag of include/rfq_hip.h): UMI
// extraction.  Part of rfq_encode_kernels.h (included from there, behind enc/rows_select.h and enc/rows_lanes.h; not a stand-alone header).
#pragma once
// Row i gives a part: bytes [tag_start[i], + tag_len[i]) of its base row, as text.  A unit - a row, with pairs the rows 2u / 2u + 1 - has the tag T: its parts, `join`
// between them where both have bytes.  The text inserted into the names of the unit's rows is X = sep, (prefix, join), T - nothing at all where T is empty -, in
// front of the name's first 0x20 byte (RFQ_TAG_AT_SPACE; a name without one: at its end) or at its end.
//   k_sel_judge_tag     sel_judge under the rule SelTagged: it validates every row's part as well and a kept name counts with |X|, so the scans carry the tagged
//                       sizes and k_sel_tables runs as it is.
//   k_tag_plan          a group of 4 lanes per OUTPUT row: where X goes (the lanes look at 64 name bytes a step) and X itself, rendered once into a record of
//                       TAG_STRIDE bytes of the context's scratch.
//   k_sel_names_tag     name_blob_find (enc/text_rows.h), then a group's bytes from three segments: the name's head, X, the name's tail.
//   k_sel_names_tag_general   RFQ_TAG=general: a thread per output name, byte by byte, straight from the names and the base rows - no plan, no scratch.
#define SL_ERR_TAG     (1u << 3)      // a part that starts below 0, has a negative length, more than RFQ_TAG_PART_MAX bases or ends behind its read   (RFQ_E_ARG)
#define SL_ERR_TAGB    (1u << 4)      // a part byte that is a code above 4 / a letter outside 0x21..0x7E                                                 (RFQ_E_DATA)
// a record of the plan: X in bytes [0, 81), zeros behind it, the insertion offset and |X| as two words at byte 88
#define TAG_STRIDE 96u
#define TAG_AT_OFF 88u
struct TagIn {
    const int32_t* tstart; const int32_t* tlen; const int32_t* lens;          // [n_rows] each
    const uint8_t* bases; uint64_t total;                                     // the base rows [n_rows][row_len]; their bytes
    uint32_t row_len, codes, pairs;                                           // (codes: the bases are A0 C1 G2 T3 N4)
    uint32_t prefix_len, sep, join, at;
    uint8_t prefix[16];
};
// The part of row i: its length, 0 for a row that gives none or whose window or length is at fault (bad: the window is; a bad LENGTH is sel_window's to report).
// start + len is formed in 64 bits.
__device__ __forceinline__ uint32_t tag_window(const TagIn& t, uint32_t i, uint32_t& start, bool& bad) {
    const int32_t l = t.lens[i]; const long long s = t.tstart[i], w = t.tlen[i];
    const bool lok = l >= 0 && (uint32_t)l <= t.row_len;
    bad = lok && (s < 0 || w < 0 || w > (long long)RFQ_TAG_PART_MAX || s + w > (long long)l);
    const bool ok = lok && !bad;
    start = ok ? (uint32_t)s : 0u;
    return ok ? (uint32_t)w : 0u;
}
// |X| of a unit whose rows give tl0 and tl1 bytes
__device__ __forceinline__ uint32_t tag_xlen(const TagIn& t, uint32_t tl0, uint32_t tl1) {
    const uint32_t T = tl0 + tl1 + ((tl0 && tl1) ? 1u : 0u);
    return T ? 1u + (t.prefix_len ? t.prefix_len + 1u : 0u) + T : 0u;
}
// a part byte that cannot be text: the tl <= 32 bytes from byte p of the base rows, in one or two 16-byte loads wherever 16 bytes from there lie inside the buffer
__device__ __forceinline__ bool tag_part_bad(const TagIn& t, uint64_t p, uint32_t tl) {
    uint32_t bad = 0;
    for (uint32_t k = 0; k < tl; k += 16u) {
        const uint32_t have = tl - k < 16u ? tl - k : 16u;
        uint32_t w[4] = { 0, 0, 0, 0 };
        if (p + k + 16u <= t.total) rt_ld16(t.bases + p + k, false, w);
        else for (uint32_t i = 0; i < have; i++) w[i >> 2] |= (uint32_t)t.bases[p + k + i] << (8u * (i & 3u));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t m = low_bytes((int)have - 4 * i);
            bad |= t.codes ? bytes_gt4(w[i] & m) : bytes_not_graph((w[i] & m) | (0x41414141u & ~m));
        }
    }
    return bad != 0;
}
// the unit of row `row`: its rows' parts (p: the part's first byte in the base rows)
struct TagUnit { uint64_t p0, p1; uint32_t tl0, tl1; };
__device__ __forceinline__ TagUnit tag_unit(const TagIn& t, uint32_t row) {
    TagUnit u; u.p1 = 0; u.tl1 = 0;
    const uint32_t r0 = t.pairs ? row & ~1u : row;
    uint32_t s; bool bad;
    u.tl0 = tag_window(t, r0, s, bad); u.p0 = (uint64_t)r0 * t.row_len + s;
    if (t.pairs) { u.tl1 = tag_window(t, r0 + 1u, s, bad); u.p1 = (uint64_t)(r0 + 1u) * t.row_len + s; }
    return u;
}
__device__ __forceinline__ uint32_t tag_base(const TagIn& t, uint64_t p) { const uint32_t c = t.bases[p]; return t.codes ? ascii4_of_code(c) & 0xFFu : c; }
// byte k of X, k < |X|
__device__ __forceinline__ uint32_t tag_x_byte(const TagIn& t, const TagUnit& u, uint32_t k) {
    if (k == 0) return t.sep;
    k -= 1u;
    if (t.prefix_len) {
        if (k < t.prefix_len) return t.prefix[k];
        if (k == t.prefix_len) return t.join;
        k -= t.prefix_len + 1u;
    }
    if (k < u.tl0) return tag_base(t, u.p0 + k);
    k -= u.tl0;
    if (u.tl0 && u.tl1) { if (k == 0) return t.join; k -= 1u; }
    return tag_base(t, u.p1 + k);
}

// ---- the judge: rfq_select_rows' rule, and the kept names grow by |X|.  Every row's own part is validated, kept or not (the mate's is its own thread's: its length is
// read here the way its window is, and counts as 0 where it is at fault - the call is refused anyway).
struct SelTagged {
    uint32_t* __restrict__ flag; uint64_t* __restrict__ nsz; const TagIn& t;
    __device__ __forceinline__ bool drops(uint32_t, uint32_t&) const { return false; }
    __device__ __forceinline__ void bad(SelStat* st, uint32_t g) const { atomicMin(&st->bad_row, (unsigned long long)g); }
    __device__ __forceinline__ void row(uint32_t g, bool kept, uint64_t nl) const { flag[g] = kept ? 1u : 0u; nsz[g] = kept ? nl : 0ull; }
    __device__ __forceinline__ void finish(SelStat*, uint32_t) const {}
    __device__ __forceinline__ uint32_t grow(uint32_t g, uint32_t, uint32_t& re) const {
        uint32_t s, ms; bool bad, mbad;
        const uint32_t tl = tag_window(t, g, s, bad);
        if (bad) re |= SL_ERR_TAG;
        else if (tl && tag_part_bad(t, (uint64_t)g * t.row_len + s, tl)) re |= SL_ERR_TAGB;
        const uint32_t tm = t.pairs ? tag_window(t, g ^ 1u, ms, mbad) : 0u;
        return tag_xlen(t, tl, tm);
    }
};
template <> struct sel_rule_grows<SelTagged> { static constexpr bool value = true; };
// grid ceil(n_rows / SJ_ROWS) x 256 threads: sel_judge's
__global__ void __launch_bounds__(256) k_sel_judge_tag(SelIn in, TagIn t, uint32_t* __restrict__ flag, uint64_t* __restrict__ nsz, SelStat* __restrict__ st) {
    SelTagged rule{ flag, nsz, t };
    sel_judge(in, st, rule);
}

// ---- the plan and the two writers follow the OUTPUT rows: output name j is input name tab[j].src with the X of that row's unit
struct TagNames {
    const uint8_t* names; const uint64_t* in_off; uint64_t names_len;         // the input blob, its [n_rows + 1] offsets and its bytes
    const SelRow* tab; uint32_t n_out;
};
#define TP_LPR 4u                     // lanes of an output row in k_tag_plan: 64 name bytes a step (an Illumina name is one step; 16 lanes per row left 12 of them idle)
#define TP_ROWS (256u / TP_LPR)       // output rows of a workgroup
// the smallest value among the TP_LPR lanes of a row, in each of them.  Called by ALL lanes of the wave.
__device__ __forceinline__ uint32_t tp_min(uint32_t v) {
#pragma unroll
    for (uint32_t d = TP_LPR / 2u; d >= 1u; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, (int)d); if (o < v) v = o; }
    return v;
}
// grid ceil(n_out / TP_ROWS) x 256 threads, TP_LPR lanes per output row.  The place: lane l looks at name bytes [64 s + 16 l, + 16) in step s - one 16-byte load at
// the name's own alignment wherever 16 bytes from there lie inside the blob, byte by byte at its very end - and the row's first hit is the minimum over its lanes;
// a wave goes on while one of its rows still looks (names of up to 64 bytes: one step).  A row without a tag is not looked at.  Then the lanes write the record, 16
// bytes at a time: lane l groups l and l + TP_LPR.
__global__ void __launch_bounds__(256) k_tag_plan(TagIn t, TagNames nm, uint8_t* __restrict__ xs) {
    const uint32_t grp = threadIdx.x / TP_LPR, gl = threadIdx.x % TP_LPR;
    const uint64_t j = (uint64_t)blockIdx.x * TP_ROWS + grp; const bool live = j < nm.n_out;
    uint64_t nbeg = 0; uint32_t nl = 0, xl = 0; TagUnit u = { 0, 0, 0, 0 };
    if (live) {
        const uint32_t src = nm.tab[j].src;
        nbeg = nm.in_off[src]; nl = (uint32_t)(nm.in_off[src + 1] - nbeg);
        u = tag_unit(t, src); xl = tag_xlen(t, u.tl0, u.tl1);
    }
    uint32_t at = nl;
    if (t.at == RFQ_TAG_AT_SPACE) {
        bool seek = live && xl != 0;
        for (uint32_t s = 0; ; s += 16u * TP_LPR) {
            const bool need = seek && s < nl;
            if (!wave_or(need ? 1u : 0u)) break;
            uint32_t first = 0xFFFFFFFFu;
            const uint32_t x = s + 16u * gl;
            if (need && x < nl) {
                const uint32_t have = nl - x < 16u ? nl - x : 16u; const uint64_t p = nbeg + x;
                uint32_t w[4] = { 0, 0, 0, 0 };
                if (p + 16u <= nm.names_len) rt_ld16(nm.names + p, false, w);
                else for (uint32_t i = 0; i < have; i++) w[i >> 2] |= (uint32_t)nm.names[p + i] << (8u * (i & 3u));
                const uint32_t m = rows_eq_bits(w, 0xFFFFFFFFu, 0x20202020u) & ((1u << have) - 1u);
                if (m) first = x + (uint32_t)__builtin_ctz(m);
            }
            first = tp_min(first);
            if (need && first != 0xFFFFFFFFu) { at = first; seek = false; }
        }
    }
    if (live) for (uint32_t x0 = 16u * gl; x0 < TAG_STRIDE; x0 += 16u * TP_LPR) {
        uint32_t w[4] = { 0, 0, 0, 0 };
        for (uint32_t i = 0; i < 16u && x0 + i < xl; i++) w[i >> 2] |= tag_x_byte(t, u, x0 + i) << (8u * (i & 3u));
        if (x0 == (TAG_AT_OFF & ~15u)) { w[2] = at; w[3] = xl; }
        *(uint4*)(xs + j * TAG_STRIDE + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// grid ceil((names_len + shift) / TN_TILE) x TN_TPB threads: name_blob_write's, over the OUTPUT blob (off[]: the output offsets, which carry the tags).  Output name g
// is bytes [0, at) of its input name, the |X| bytes of its record, the input name from `at` on.  A whole group inside one segment of one name is one 16-byte load - of
// the name at its own alignment, of X from the one or two aligned groups of the record that hold it - and one aligned store; any other group is put together byte
// by byte in registers.
struct TagNameOf {
    const uint8_t* p0; const uint8_t* rec; uint32_t at, xl;
    __device__ __forceinline__ TagNameOf(const TagNames& nm, const uint8_t* xs, uint32_t g) {
        p0 = nm.names + nm.in_off[nm.tab[g].src]; rec = xs + (uint64_t)g * TAG_STRIDE;
        const uint2 ax = *(const uint2*)(rec + TAG_AT_OFF); at = ax.x; xl = ax.y;
    }
    __device__ __forceinline__ uint32_t byte(uint64_t o) const { return o < at ? p0[o] : (o < (uint64_t)at + xl ? rec[o - at] : p0[o - xl]); }
};
__global__ void __launch_bounds__(TN_TPB) k_sel_names_tag(TagNames nm, const uint8_t* __restrict__ xs, const uint64_t* __restrict__ off, uint8_t* __restrict__ blob, uint64_t names_len) {
    NameGroup G;
    if (!name_blob_find(off, nm.n_out, blob, names_len, G)) return;
    uint32_t g = G.g; uint64_t beg = off[g], end = off[g + 1];
    TagNameOf n(nm, xs, g);
    if (G.qe - G.qa == 16u && G.qe <= end) {
        const uint64_t o = G.qa - beg; const uint8_t* s = nullptr; bool in_rec = false;
        if (o + 16u <= n.at) s = n.p0 + o;
        else if (o >= (uint64_t)n.at + n.xl) s = n.p0 + (o - n.xl);
        else if (o >= n.at && o + 16u <= (uint64_t)n.at + n.xl) { s = n.rec + (o - n.at); in_rec = true; }
        if (s) {
            uint32_t w[4]; rt_ld16(s, in_rec, w);
            *(uint4*)(G.nb + G.A) = make_uint4(w[0], w[1], w[2], w[3]);
            return;
        }
    }
    unsigned long long h0 = 0, h1 = 0; const uint32_t nby = (uint32_t)(G.qe - G.qa);
    for (uint32_t i = 0; i < nby; i++) {
        const uint64_t q = G.qa + i;
        while (q >= end) { g++; beg = end; end = off[g + 1]; n = TagNameOf(nm, xs, g); }
        const unsigned long long c = n.byte(q - beg);
        if (i < 8u) h0 |= c << (8u * i); else h1 |= c << (8u * (i - 8u));
    }
    name_group_store(G, blob, h0, h1);
}

// grid ceil(n_out / 256) x 256 threads, a thread per output name: the place by a walk over the name, then head, X and tail byte by byte
__global__ void __launch_bounds__(256) k_sel_names_tag_general(TagIn t, TagNames nm, const uint64_t* __restrict__ off, uint8_t* __restrict__ blob) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= nm.n_out) return;
    const uint32_t src = nm.tab[j].src;
    const uint64_t nbeg = nm.in_off[src], nl = nm.in_off[src + 1] - nbeg;
    const TagUnit u = tag_unit(t, src); const uint32_t xl = tag_xlen(t, u.tl0, u.tl1);
    uint64_t at = nl;
    if (xl && t.at == RFQ_TAG_AT_SPACE) for (uint64_t i = 0; i < nl; i++) if (nm.names[nbeg + i] == 0x20u) { at = i; break; }
    uint8_t* o = blob + off[j];
    for (uint64_t i = 0; i < at; i++) o[i] = nm.names[nbeg + i];
    for (uint32_t k = 0; k < xl; k++) o[at + k] = (uint8_t)tag_x_byte(t, u, k);
    for (uint64_t i = at; i < nl; i++) o[xl + i] = nm.names[nbeg + i];
}
