// merge_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_merge_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/merge_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   merge_asan_main         the shapes of tests/_merge.py - random pairs over the row strides 1 .. 260, buffer shifts 0 / 1 on both sides, both base modes, both output
//   strides, the default path and RFQ_MERGE=general - and every insert of its seven (l1, l2), with rows in allocations that end where the rows end and outputs of
//   exactly their size, compared with a host loop written from include/rfq_hip.h; then every refusal, each followed by a good call.
//   Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <string>
#include <vector>

struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, Q, names; std::vector<int32_t> lens, insert; std::vector<uint64_t> off; };
static uint32_t cls_of(uint8_t b, int codes) {
    if (codes) return b < 4 ? b : 4;
    switch (b) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
static uint8_t comp_of(uint8_t b, int codes) {
    if (codes) return b < 4 ? (uint8_t)(3 - b) : b;
    const char* from = "ATCGatcg"; const char* to = "TAGCtagc";
    for (int i = 0; i < 8; i++) if (b == (uint8_t)from[i]) return (uint8_t)to[i];
    return b;
}
static uint8_t any_base(int codes) { return codes ? (uint8_t)"\0\1\2\3\0\1\2\3\4\7\377"[rnd() % 11] : (uint8_t)"ACGTACGTacgtNnRY."[rnd() % 17]; }
// pairs at stride L: lengths 1 .. L (l1 / l2 > 0: those), bases of every class, scores with many ties, noise behind the reads, names of 0 .. 20 bytes; insert: -1
// for every third pair, else a random valid one (every > 0: pair k gets insert k + 1)
static Rows make_rows(uint32_t pairs, uint32_t L, int codes, uint32_t l1 = 0, uint32_t l2 = 0, bool every = false) {
    Rows r; r.n = 2 * pairs; r.L = L; r.codes = codes; r.B.resize((size_t)r.n * L); r.Q.resize((size_t)r.n * L); r.lens.resize(r.n); r.insert.resize(pairs); r.off.assign(1, 0);
    for (uint32_t i = 0; i < r.n; i++) {
        const uint32_t l = (i & 1) ? (l2 ? l2 : 1 + rnd() % L) : (l1 ? l1 : 1 + rnd() % L);
        r.lens[i] = (int32_t)l;
        for (uint32_t j = 0; j < L; j++) {
            r.B[(size_t)i * L + j] = j < l ? any_base(codes) : (uint8_t)rnd();
            r.Q[(size_t)i * L + j] = (j < l && rnd() % 3 == 0) ? (uint8_t)30 : (uint8_t)rnd();
        }
        if ((i & 1) && (i / 2) % 2 == 0)                                     // most of this pair agrees at insert = min(l1, l2)
            for (uint32_t j = 0, m = std::min<uint32_t>(l, (uint32_t)r.lens[i - 1]); j < m; j++) r.B[(size_t)i * L + j] = comp_of(r.B[(size_t)(i - 1) * L + (m - 1 - j)], codes);
        for (uint32_t j = 0, nl = rnd() % 21; j < nl; j++) r.names.push_back((uint8_t)(33 + rnd() % 90));
        r.off.push_back(r.names.size());
    }
    for (uint32_t k = 0; k < pairs; k++) {
        const uint32_t a = (uint32_t)r.lens[2 * k], b = (uint32_t)r.lens[2 * k + 1];
        r.insert[k] = every ? (int32_t)(k + 1) : (k % 3 == 2 ? -1 : (k % 4 == 0 ? (int32_t)std::min(a, b) : (int32_t)(1 + rnd() % (a + b - 1))));
    }
    return r;
}

struct Ref { std::vector<uint8_t> B, Q, names; std::vector<int32_t> lens; std::vector<uint64_t> off; rfq_merge_rows_result s; };
// the rules of include/rfq_hip.h as plain loops; the rows at stride L_out, padded
static Ref reference(const Rows& r, uint32_t L_out, uint8_t pad_b, uint8_t pad_q) {
    Ref o; memset(&o.s, 0, sizeof o.s); o.s.n_pairs = r.n / 2; o.off.assign(1, 0);
    for (uint32_t k = 0; k < r.n / 2; k++) if (r.insert[k] >= 0) o.s.max_len = std::max(o.s.max_len, (uint32_t)r.insert[k]);
    for (uint32_t k = 0; k < r.n / 2; k++) {
        const int64_t ins = r.insert[k], l1 = r.lens[2 * k], l2 = r.lens[2 * k + 1];
        if (ins < 0) continue;
        const uint8_t* r1 = &r.B[(size_t)(2 * k) * r.L]; const uint8_t* q1 = &r.Q[(size_t)(2 * k) * r.L]; const uint8_t* r2 = r1 + r.L; const uint8_t* q2 = q1 + r.L;
        const size_t at = o.B.size(); o.B.resize(at + L_out, pad_b); o.Q.resize(at + L_out, pad_q);
        for (int64_t p = 0; p < ins; p++) {
            const bool c1 = p < std::min(l1, ins), c2 = p >= ins - l2;
            const uint8_t x1 = c1 ? r1[p] : 0, y1 = c1 ? q1[p] : 0, x2 = c2 ? comp_of(r2[ins - 1 - p], r.codes) : 0, y2 = c2 ? q2[ins - 1 - p] : 0;
            uint8_t b, q;
            if (c1 && c2) {
                o.s.overlap_bases++;
                const uint32_t k1 = cls_of(x1, r.codes), k2 = cls_of(x2, r.codes);
                if (k1 < 4 && k1 == k2) { b = x1; q = std::max(y1, y2); }
                else if ((k1 < 4) != (k2 < 4)) { b = k1 < 4 ? x1 : x2; q = k1 < 4 ? y1 : y2; }
                else if (y1 >= y2) { b = x1; q = (uint8_t)(y1 - y2); }
                else { b = x2; q = (uint8_t)(y2 - y1); }
            } else if (c1) { b = x1; q = y1; } else { b = x2; q = y2; }
            o.B[at + p] = b; o.Q[at + p] = q;
        }
        o.lens.push_back((int32_t)ins); o.s.n_rows++; o.s.n_bases += ins;
        const uint64_t a = r.off[2 * k], e = r.off[2 * k + 1];
        o.names.insert(o.names.end(), r.names.begin() + a, r.names.begin() + e); o.off.push_back(o.names.size());
        o.s.max_name = std::max(o.s.max_name, (uint32_t)(e - a));
    }
    o.s.names_len = o.names.size();
    return o;
}

static rfq_rows_in rows_in(const Rows& r, const Dev& b, const Dev& q, const Dev& l, const Dev& nm, const Dev& off) {
    rfq_rows_in in = rows_in(r.n, r.L, r.codes, b, &q, l);
    in.d_names = nm.p; in.names_len = r.names.size(); in.d_name_off = (const uint64_t*)off.p;
    return in;
}
// a size query and a write into buffers of exactly the reported sizes, both against the host loop
static int run(rfq_ctx* ctx, const char* what, const Rows& r, bool x16, size_t shift) {
    const uint8_t pad_b = 0xA7, pad_q = 0x51;
    Dev db(ctx, r.B.data(), r.B.size(), shift), dq(ctx, r.Q.data(), r.Q.size(), shift), dl(ctx, r.lens.data(), r.n * 4ull), dn(ctx, r.names.data(), r.names.size(), shift),
        doff(ctx, r.off.data(), r.off.size() * 8ull), di(ctx, r.insert.data(), r.insert.size() * 4ull);
    const rfq_rows_in in = rows_in(r, db, dq, dl, dn, doff);
    rfq_merge_rows_args a; memset(&a, 0, sizeof a); a.d_insert = (const int32_t*)di.p;
    rfq_merge_rows_result q, g;
    if (rfq_merge_rows(ctx, &in, &a, &q)) return fail(what, rfq_last_error(ctx));
    const uint32_t L = x16 ? (q.max_len + 15u) / 16u * 16u + 16u : std::max(q.max_len, 1u);
    const Ref e = reference(r, L, pad_b, pad_q);
    if (memcmp(&q, &e.s, sizeof q)) return fail(what, "the size query's result differs from the host's");
    const size_t m = (size_t)q.n_rows;
    Dev ob(ctx, nullptr, m * L, shift), oq(ctx, nullptr, m * L, shift), ol(ctx, nullptr, m * 4), on(ctx, nullptr, (size_t)q.names_len, shift), oo(ctx, nullptr, (m + 1) * 8);
    a.row_len = L; a.pad_base = pad_b; a.pad_qual = pad_q; a.d_bases = ob.p; a.bases_cap = m * L; a.d_quals = oq.p; a.quals_cap = m * L; a.d_lens = (int32_t*)ol.p; a.lens_cap = m;
    a.d_names = on.p; a.names_cap = (size_t)q.names_len; a.d_name_off = (uint64_t*)oo.p; a.off_cap = m + 1;
    if (rfq_merge_rows(ctx, &in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e.s, sizeof g)) return fail(what, "the result differs from the host's");
    std::vector<uint8_t> hb(m * L + 1), hq(m * L + 1), hn(e.names.size() + 1); std::vector<int32_t> hl(m + 1); std::vector<uint64_t> ho(m + 1);
    rfq_copy_d2h(ctx, ho.data(), oo.p, (m + 1) * 8);
    if (memcmp(ho.data(), e.off.data(), (m + 1) * 8)) return fail(what, "the name offsets differ");
    if (m) {
        rfq_copy_d2h(ctx, hb.data(), ob.p, m * L); rfq_copy_d2h(ctx, hq.data(), oq.p, m * L); rfq_copy_d2h(ctx, hl.data(), ol.p, m * 4);
        if (memcmp(hb.data(), e.B.data(), m * L)) return fail(what, "the base rows differ");
        if (memcmp(hq.data(), e.Q.data(), m * L)) return fail(what, "the quality rows differ");
        if (memcmp(hl.data(), e.lens.data(), m * 4)) return fail(what, "lens differ");
    }
    if (!e.names.empty()) { rfq_copy_d2h(ctx, hn.data(), on.p, e.names.size()); if (memcmp(hn.data(), e.names.data(), e.names.size())) return fail(what, "the name blob differs"); }
    return 0;
}

static int good(rfq_ctx* ctx) { const Rows r = make_rows(12, 20, 1); return run(ctx, "a good call after a refusal", r, false, 0); }
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_merge_rows_args& a, const char* needle) {
    rfq_merge_rows_result g;
    const int rc = rfq_merge_rows(ctx, &in, &a, &g);
    if (rc != RFQ_E_ARG) return fail(what, "not refused with RFQ_E_ARG");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, host_refusals = 0, device_refusals = 0;
    const uint32_t strides[] = { 1, 15, 16, 17, 33, 64, 152, 260 }; const uint32_t every[][2] = { { 1, 1 }, { 16, 16 }, { 20, 20 }, { 17, 33 }, { 33, 17 }, { 40, 5 }, { 5, 40 } };
    for (int general = 0; general < 2 && !bad; general++) {
        if (rfq_set_option(ctx, "RFQ_MERGE", general ? "general" : nullptr)) return fail("RFQ_MERGE", rfq_last_error(ctx));
        for (uint32_t L : strides) for (int codes = 0; codes < 2; codes++) for (size_t shift = 0; shift < 2; shift++) for (int x16 = 0; x16 < 2 && !bad; x16++) {
            const Rows r = make_rows(36, L, codes);
            char what[128]; snprintf(what, sizeof what, "general %d row_len %u codes %d shift %zu x16 %d", general, L, codes, shift, x16);
            bad |= run(ctx, what, r, x16 != 0, shift); calls++;
        }
        for (const auto& e : every) for (int codes = 0; codes < 2; codes++) for (size_t shift = 0; shift < 2; shift++) for (int x16 = 0; x16 < 2 && !bad; x16++) {
            const Rows r = make_rows(e[0] + e[1] - 1, std::max(e[0], e[1]), codes, e[0], e[1], true);
            char what[128]; snprintf(what, sizeof what, "general %d every insert of (%u, %u) codes %d shift %zu x16 %d", general, e[0], e[1], codes, shift, x16);
            bad |= run(ctx, what, r, x16 != 0, shift); calls++;
        }
    }
    rfq_set_option(ctx, "RFQ_MERGE", nullptr);
    { const Rows z = make_rows(0, 16, 0); bad |= run(ctx, "no rows", z, false, 0); calls++; }
    { Rows z = make_rows(9, 16, 0); std::fill(z.insert.begin(), z.insert.end(), -1); bad |= run(ctx, "no pair merged", z, false, 0); calls++; }
    if (!bad) {   // the refusals
        const Rows r = make_rows(20, 16, 1);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);                   // (a word more: the misaligned pointers stay inside it)
        std::vector<int32_t> ip = r.insert; ip.push_back(0);
        std::vector<uint64_t> fp = r.off; fp.push_back(0);
        Dev db(ctx, r.B.data(), r.B.size()), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, lp.data(), lp.size() * 4), dn(ctx, r.names.data(), r.names.size()),
            doff(ctx, fp.data(), fp.size() * 8), di(ctx, ip.data(), ip.size() * 4), out(ctx, nullptr, 1 << 16);
        const rfq_rows_in in = rows_in(r, db, dq, dl, dn, doff);
        rfq_merge_rows_args base; memset(&base, 0, sizeof base); base.d_insert = (const int32_t*)di.p;
        rfq_merge_rows_args w = base; w.row_len = 32; w.d_bases = out.p; w.bases_cap = 20 * 32;
        rfq_merge_rows_args a; rfq_rows_in x;
#define REFUSED(WHAT, IN, A, NEEDLE) { bad |= refused(ctx, WHAT, IN, A, NEEDLE); host_refusals++; }
        x = in; x.n_rows = 39; REFUSED("odd n_rows", x, base, "pairs")
        a = base; a.d_insert = nullptr; REFUSED("no d_insert", in, a, "d_insert")
        a = base; a.d_insert = (const int32_t*)(di.p + 2); REFUSED("misaligned d_insert", in, a, "aligned")
        a = base; a.row_len = 32; a.d_lens = (int32_t*)(out.p + 2); a.lens_cap = 100; REFUSED("misaligned d_lens", in, a, "aligned")
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); REFUSED("misaligned rows->d_lens", x, base, "aligned")
        a = base; a.row_len = 32; a.d_name_off = (uint64_t*)(out.p + 4); a.off_cap = 100; REFUSED("misaligned d_name_off", in, a, "aligned")
        x = in; x.d_name_off = (const uint64_t*)(doff.p + 4); REFUSED("misaligned rows->d_name_off", x, base, "aligned")
        a = w; a.row_len = 0; REFUSED("row_len 0", in, a, "row_len")
        x = in; x.base_mode = 2; REFUSED("bad base_mode", x, base, "base_mode")
        x = in; x.d_bases = nullptr; REFUSED("no bases with bases wanted", x, w, "d_bases")
        x = in; x.d_quals = nullptr; a = base; a.row_len = 32; a.d_quals = out.p; a.quals_cap = 20 * 32; REFUSED("no quals with quals wanted", x, a, "d_quals")
        x = in; x.d_name_off = nullptr; x.d_names = nullptr; a = base; a.row_len = 32; a.d_names = out.p; a.names_cap = 4096; REFUSED("names wanted of rows without names", x, a, "without names")
        a = w; a.d_bases = db.p; REFUSED("bases out on bases in", in, a, "overlaps")
        a = base; a.row_len = 32; a.d_quals = dq.p + 40 * 16 - 1; a.quals_cap = 20 * 32; REFUSED("quals out on the last quality in", in, a, "overlaps")
        a = base; a.row_len = 32; a.d_lens = (int32_t*)dl.p; a.lens_cap = 20; REFUSED("lens out on lens in", in, a, "overlaps")
        a = base; a.row_len = 32; a.d_lens = (int32_t*)di.p; a.lens_cap = 20; REFUSED("lens out on d_insert", in, a, "overlaps")
        a = base; a.row_len = 32; a.d_name_off = (uint64_t*)doff.p; a.off_cap = 21; REFUSED("offsets out on offsets in", in, a, "overlaps")
#undef REFUSED
        // device-side: (what, needle, the change)
        for (int general = 0; general < 2; general++) for (int which = 0; which < 8; which++) {
            std::vector<int32_t> l2 = r.lens, i2 = r.insert; std::vector<uint64_t> f2 = r.off; size_t nl = r.names.size();
            for (auto& v : l2) v = std::max(v, 3);
            for (auto& v : i2) v = v >= 0 ? 2 : -1;
            char needle[64];
            switch (which) {
            case 0: l2[17] = -1; snprintf(needle, sizeof needle, "first such row: 17)"); break;
            case 1: l2[38] = 17; snprintf(needle, sizeof needle, "first such row: 38)"); break;
            case 2: i2[4] = 0; snprintf(needle, sizeof needle, "first such pair: 4)"); break;
            case 3: i2[9] = l2[18] + l2[19]; snprintf(needle, sizeof needle, "first such pair: 9)"); break;
            case 4: l2[12] = 0; i2[6] = 1; snprintf(needle, sizeof needle, "first such pair: 6)"); break;
            case 5: f2[12] = f2[13] + 1; snprintf(needle, sizeof needle, "first such row: 12)"); break;
            case 6: nl -= 1; snprintf(needle, sizeof needle, "first such row: 39)"); break;
            default: l2[11] = 23; snprintf(needle, sizeof needle, "first such row: 11)"); break;      // (pair 5 is not merged)
            }
            if (which == 6 && f2[40] == 0) continue;
            Dev d2(ctx, l2.data(), 160), d3(ctx, i2.data(), 80), d4(ctx, f2.data(), 41 * 8);
            x = in; x.d_lens = (const int32_t*)d2.p; x.d_name_off = (const uint64_t*)d4.p; x.names_len = nl;
            a = w; a.d_insert = (const int32_t*)d3.p;
            rfq_set_option(ctx, "RFQ_MERGE", general ? "general" : nullptr);
            rfq_merge_rows_result g;
            if (rfq_merge_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a device-side refusal", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_MERGE", nullptr);
            bad |= good(ctx); device_refusals++;
        }
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("merge_asan: %d good calls (8 row strides and every insert of 7 length pairs x 2 base modes x 2 shifts x 2 output strides x 2 paths, no rows, no pair merged), "
           "%d host and %d device refusals each followed by a good call: all as the host loop says, no sanitizer report\n", calls, host_refusals, device_refusals);
    return 0;
}
