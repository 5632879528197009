// select_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_select_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/select_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   select_asan_main        the good shapes of tests/_select.py - windows at every residue over the row strides 1 .. 160 and buffer shifts 0 / 1 / 7 / 15, the mask
//   patterns over 0 .. 2049 rows, a scan of 16385 rows, pairs and min_len, names at every residue, a name longer than a tile, rows without names - into caller buffers
//   of exactly the reported sizes (every allocation ends where its data ends), compared with a host reference; then the refusals, each followed by a good call.
//   Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <string>
#include <vector>

struct Rows {
    uint32_t n = 0, L = 1; std::vector<uint8_t> B, Q; std::vector<int32_t> lens; std::vector<std::string> names; bool named = true;
    std::vector<uint8_t> keep; std::vector<int32_t> start, len; bool has_keep = false, has_start = false, has_len = false;
};
static Rows make_rows(uint32_t n, uint32_t L, bool full, uint32_t name_mod) {
    Rows r; r.n = n; r.L = L; r.B.resize((size_t)n * L); r.Q.resize((size_t)n * L); r.lens.resize(n); r.names.resize(n);
    for (auto& x : r.B) x = (uint8_t)rnd();
    for (auto& x : r.Q) x = (uint8_t)rnd();
    for (uint32_t i = 0; i < n; i++) { r.lens[i] = full ? (int32_t)L : 1 + (int32_t)(rnd() % L); r.names[i] = std::string(1 + (i * 7 + i / 40) % name_mod, (char)('a' + i % 26)); }
    return r;
}

// one size query and one call into exact buffers, against the host's own selection; rule: 0 the longest window, 1 one more, 2 the next multiple of 16
static int run(rfq_ctx* ctx, const char* what, const Rows& r, int pairs, uint32_t min_len, int rule, size_t in_shift, size_t out_shift) {
    const uint32_t n = r.n;
    std::vector<uint64_t> off(n + 1, 0); std::string blob;
    for (uint32_t i = 0; i < n; i++) { blob += r.names[i]; off[i + 1] = blob.size(); }
    // host reference
    std::vector<int> why(n, 0); std::vector<int64_t> st(n), ln(n);
    for (uint32_t i = 0; i < n; i++) { st[i] = r.has_start ? r.start[i] : 0; ln[i] = r.has_len ? r.len[i] : r.lens[i] - st[i];
        why[i] = (r.has_keep && !r.keep[i]) ? 1 : (ln[i] < (int64_t)min_len ? 2 : 0); }
    std::vector<uint32_t> idx; uint64_t cnt[4] = { 0, 0, 0, 0 };
    for (uint32_t i = 0; i < n; i++) { int w = why[i]; if (!w && pairs && why[i ^ 1]) w = 3; cnt[w]++; if (!w) idx.push_back(i); }
    uint32_t ml = 0, mn = 0; uint64_t nb = 0, nl = 0;
    for (uint32_t i : idx) { if (ln[i] > ml) ml = (uint32_t)ln[i]; nb += (uint64_t)ln[i]; if (r.named) { nl += r.names[i].size(); if (r.names[i].size() > mn) mn = (uint32_t)r.names[i].size(); } }
    const uint32_t m = (uint32_t)idx.size();
    Dev db(ctx, r.B.data(), r.B.size(), in_shift), dq(ctx, r.Q.data(), r.Q.size(), in_shift), dl(ctx, r.lens.data(), n * 4ull);
    Dev dn(ctx, blob.data(), blob.size(), in_shift), dof(ctx, off.data(), off.size() * 8);
    Dev dk(ctx, r.keep.data(), r.has_keep ? n : 0), ds(ctx, r.start.data(), r.has_start ? n * 4ull : 0), dw(ctx, r.len.data(), r.has_len ? n * 4ull : 0);
    rfq_rows_in in = rows_in(n, r.L, 0, db, &dq, dl);
    if (r.named) { in.d_names = dn.p; in.names_len = blob.size(); in.d_name_off = (const uint64_t*)dof.p; }
    rfq_select_rows_args a; memset(&a, 0, sizeof a); rfq_select_rows_result q, g;
    a.d_keep = r.has_keep ? dk.p : nullptr; a.d_start = r.has_start ? (const int32_t*)ds.p : nullptr; a.d_len = r.has_len ? (const int32_t*)dw.p : nullptr;
    a.pairs = pairs; a.min_len = min_len;
    if (rfq_select_rows(ctx, &in, &a, &q)) return fail(what, rfq_last_error(ctx));
    if (q.n_rows != m || q.n_bases != nb || q.names_len != nl || q.max_len != ml || q.max_name != mn || q.n_in != n || q.dropped_mask != cnt[1] || q.dropped_short != cnt[2] ||
        q.dropped_mate != cnt[3]) return fail(what, "the size query disagrees with the host");
    const uint32_t L = rule == 0 ? (ml ? ml : 1) : (rule == 1 ? ml + 1 : (ml / 16 + 1) * 16);
    const size_t rb = (size_t)m * L;
    Dev ob(ctx, nullptr, rb, out_shift), oq(ctx, nullptr, rb, out_shift), ol(ctx, nullptr, m * 4ull), on(ctx, nullptr, (size_t)nl, out_shift), oo(ctx, nullptr, (m + 1) * 8ull);
    a.row_len = L; a.pad_base = 0xA7; a.pad_qual = 0x51;
    a.d_bases = ob.p; a.bases_cap = rb; a.d_quals = oq.p; a.quals_cap = rb; a.d_lens = (int32_t*)ol.p; a.lens_cap = m;
    if (r.named) { a.d_names = on.p; a.names_cap = (size_t)nl; a.d_name_off = (uint64_t*)oo.p; a.off_cap = m + 1; }
    if (rfq_select_rows(ctx, &in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &q, sizeof g)) return fail(what, "the call's result differs from the size query's");
    std::vector<uint8_t> hb(rb + 1), hq(rb + 1), hn((size_t)nl + 1); std::vector<int32_t> hl(m + 1); std::vector<uint64_t> ho(m + 1);
    rfq_copy_d2h(ctx, hb.data(), ob.p, rb); rfq_copy_d2h(ctx, hq.data(), oq.p, rb); rfq_copy_d2h(ctx, hl.data(), ol.p, m * 4ull);
    if (r.named) { rfq_copy_d2h(ctx, hn.data(), on.p, (size_t)nl); rfq_copy_d2h(ctx, ho.data(), oo.p, (m + 1) * 8ull); }
    uint64_t at = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = idx[j];
        if (hl[j] != (int32_t)ln[i]) return fail(what, "a length differs");
        for (uint32_t k = 0; k < L; k++) {
            const uint8_t wb = k < ln[i] ? r.B[(size_t)i * r.L + st[i] + k] : 0xA7, wq = k < ln[i] ? r.Q[(size_t)i * r.L + st[i] + k] : 0x51;
            if (hb[(size_t)j * L + k] != wb || hq[(size_t)j * L + k] != wq) return fail(what, "a row byte differs");
        }
        if (r.named) { if (ho[j] != at || memcmp(hn.data() + at, r.names[i].data(), r.names[i].size())) return fail(what, "a name differs"); at += r.names[i].size(); }
    }
    if (r.named && ho[m] != nl) return fail(what, "the last offset differs");
    return 0;
}

static int good(rfq_ctx* ctx) {
    Rows r = make_rows(70, 20, false, 3);
    r.has_keep = true; r.keep.resize(70); for (uint32_t i = 0; i < 70; i++) r.keep[i] = i % 5 != 2;
    return run(ctx, "the good call behind a refusal", r, 1, 1, 0, 0, 0);
}

static int shapes(rfq_ctx* ctx) {
    int bad = 0; char what[128];
    const uint32_t strides[] = { 1, 15, 16, 17, 33, 150, 160 }; const size_t shifts[][2] = { { 0, 0 }, { 1, 7 }, { 7, 1 }, { 15, 15 }, { 0, 1 }, { 15, 0 } };
    for (uint32_t L : strides) {                                             // test 2: every start in 0..min(17, L), every end from there to L
        std::vector<int32_t> s, w;
        for (uint32_t a = 0; a <= (L < 17 ? L : 17); a++) for (uint32_t e = a; e <= L; e += (L > 40 && e > a + 20 && e + 20 < L ? 7 : 1)) { s.push_back((int32_t)a); w.push_back((int32_t)(e - a)); }
        Rows r = make_rows((uint32_t)s.size(), L, true, 3); r.has_start = r.has_len = true; r.start = s; r.len = w;
        for (int rule = 0; rule < 3; rule++) for (auto& sh : shifts) {
            snprintf(what, sizeof what, "windows: stride %u, rule %d, shifts %zu / %zu", L, rule, sh[0], sh[1]);
            bad |= run(ctx, what, r, 0, 0, rule, sh[0], sh[1]);
        }
        r.has_len = false;
        for (uint32_t i = 0; i < r.n; i++) { int32_t l = (int32_t)L - (int32_t)(i % 3); r.lens[i] = l < r.start[i] ? r.start[i] : l; }
        bad |= run(ctx, "windows to the end of the read", r, 0, 0, 2, 0, 0);
    }
    const uint32_t counts[] = { 0, 1, 2, 255, 256, 257, 2049 };
    for (uint32_t n : counts) for (int pat = 0; pat < 7; pat++) {             // test 3
        Rows r = make_rows(n, 20, false, 3); r.has_keep = true; r.keep.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const bool k = pat == 0 ? true : pat == 1 ? false : pat == 2 ? i == 0 : pat == 3 ? i + 1 == n : pat == 4 ? (i & 1) : pat == 5 ? (i >= 250 && i < 262) : (rnd() & 1);
            const uint8_t v[4] = { 1, 0xFF, 2, 0x80 }; r.keep[i] = k ? v[i % 4] : 0;
        }
        snprintf(what, sizeof what, "masks: %u rows, pattern %d", n, pat);
        bad |= run(ctx, what, r, 0, 1, n % 2 ? 2 : 0, 0, 0);
    }
    {   // test 4: the tiled scan
        Rows r = make_rows(16385, 4, false, 2); r.has_keep = true; r.keep.resize(r.n); for (auto& k : r.keep) k = rnd() & 1;
        for (auto& nm : r.names) nm += "x";
        bad |= run(ctx, "scan: 16385 rows", r, 0, 1, 0, 0, 0);
    }
    {   // test 5: pairs and min_len
        Rows r = make_rows(24, 40, true, 3); r.has_keep = r.has_start = r.has_len = true; r.keep.assign(24, 1); r.start.assign(24, 0); r.len.assign(24, 40);
        r.keep[3] = r.keep[4] = r.keep[6] = r.keep[7] = r.keep[13] = 0; r.len[9] = r.len[10] = 9; r.len[12] = 0;
        bad |= run(ctx, "pairs, min_len 10", r, 1, 10, 0, 0, 0); bad |= run(ctx, "no pairs, min_len 10", r, 0, 10, 0, 0, 0);
        r.keep.assign(24, 1); r.len.assign(24, 40); r.len[3] = 0; r.start[3] = 40;
        bad |= run(ctx, "an empty window, min_len 0", r, 1, 0, 0, 0, 0); bad |= run(ctx, "an empty window, min_len 1", r, 1, 1, 0, 0, 0);
    }
    {   // test 6: names at every residue, a name longer than a tile (kept, dropped), names of no bytes, rows without names
        Rows r = make_rows(640, 8, false, 40); r.has_keep = true; r.keep.resize(640); for (uint32_t i = 0; i < 640; i++) r.keep[i] = i % 3 != 1;
        for (auto& sh : shifts) bad |= run(ctx, "names at every residue", r, 0, 1, 0, sh[0], sh[1]);
        for (uint32_t i = 100; i < 140; i++) r.names[i].clear();
        bad |= run(ctx, "names of no bytes", r, 0, 1, 0, 0, 3);
        Rows t = make_rows(40, 8, false, 33); t.names[20] = std::string(5000, 'L'); t.has_keep = true; t.keep.assign(40, 1); t.keep[3] = 0;
        bad |= run(ctx, "a long name kept", t, 0, 1, 0, 0, 5); t.keep[20] = 0; bad |= run(ctx, "a long name dropped", t, 0, 1, 0, 9, 0);
        t.named = false; bad |= run(ctx, "rows without names", t, 0, 1, 2, 1, 1);
    }
    return bad;
}

static int refusals(rfq_ctx* ctx) {
    int bad = 0;
    const uint32_t n = 60, L = 24;
    Rows r = make_rows(n, L, false, 9);
    for (auto& l : r.lens) if (l < 4) l = 4;
    r.lens[1] = (int32_t)L;                                                  // (the longest window is L - 2)
    std::vector<uint64_t> off(n + 1, 0); std::string blob;
    for (uint32_t i = 0; i < n; i++) { blob += r.names[i]; off[i + 1] = blob.size(); }
    std::vector<int32_t> start(n, 1), len(n); for (uint32_t i = 0; i < n; i++) len[i] = r.lens[i] - 2;
    struct Case { const char* what; int code; int which; uint32_t row; int64_t v; } cases[] = {
        { "start = -1", RFQ_E_ARG, 1, 17, -1 }, { "start = lens + 1", RFQ_E_ARG, 1, 23, -2 }, { "start + len = lens + 1", RFQ_E_ARG, 2, 5, -3 },
        { "start = len = INT32_MAX", RFQ_E_ARG, 3, 31, 0x7FFFFFFF }, { "lens = row_len + 1", RFQ_E_ARG, 0, 44, L + 1 }, { "lens = -1", RFQ_E_ARG, 0, 0, -1 },
        { "decreasing name offsets", RFQ_E_ARG, 4, 12, 0 }, { "odd rows with pairs", RFQ_E_ARG, 5, 0, 0 }, { "misaligned d_lens", RFQ_E_ARG, 6, 0, 0 },
        { "misaligned d_name_off", RFQ_E_ARG, 7, 0, 0 }, { "an output on an input", RFQ_E_ARG, 8, 0, 0 }, { "row_len one short", RFQ_E_NOSPACE, 9, 0, 0 },
        { "bases_cap one short", RFQ_E_NOSPACE, 10, 0, 0 }, { "names_cap one short", RFQ_E_NOSPACE, 11, 0, 0 }, { "off_cap one short", RFQ_E_NOSPACE, 12, 0, 0 } };
    for (const Case& c : cases) {
        std::vector<int32_t> lens = r.lens, s = start, w = len; std::vector<uint64_t> o = off; bool len_null = false;
        if (c.which == 0) lens[c.row] = (int32_t)c.v;
        if (c.which == 1) { s[c.row] = c.v == -2 ? lens[c.row] + 1 : (int32_t)c.v; len_null = c.v == -2; }
        if (c.which == 2) { s[c.row] = 3; w[c.row] = lens[c.row] - 2; }
        if (c.which == 3) { s[c.row] = w[c.row] = (int32_t)c.v; }
        if (c.which == 4) std::swap(o[12], o[13]);
        Dev db(ctx, r.B.data(), r.B.size()), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, lens.data(), n * 4ull), dn(ctx, blob.data(), blob.size()), dof(ctx, o.data(), o.size() * 8);
        Dev ds(ctx, s.data(), n * 4ull), dw(ctx, w.data(), n * 4ull);
        const size_t rb = (size_t)n * L;
        Dev ob(ctx, nullptr, rb), oq(ctx, nullptr, rb), ol(ctx, nullptr, n * 4ull), on(ctx, nullptr, blob.size()), oo(ctx, nullptr, (n + 1) * 8ull);
        rfq_rows_in in = rows_in(c.which == 5 ? n - 1 : n, L, 0, db, &dq, dl);
        if (c.which == 6) in.d_lens = (const int32_t*)(dl.p + 2);
        in.d_names = dn.p; in.names_len = blob.size(); in.d_name_off = (const uint64_t*)(dof.p + (c.which == 7 ? 4 : 0));
        rfq_select_rows_args a; memset(&a, 0, sizeof a); rfq_select_rows_result g;
        a.d_start = (const int32_t*)ds.p; a.d_len = len_null ? nullptr : (const int32_t*)dw.p; a.pairs = c.which == 5; a.min_len = 1;
        a.row_len = c.which == 9 ? L - 3 : L; a.pad_base = a.pad_qual = 0xFF;
        a.d_bases = c.which == 8 ? (uint8_t*)db.p + 5 : ob.p; a.bases_cap = rb - (c.which == 10); a.d_quals = oq.p; a.quals_cap = rb; a.d_lens = (int32_t*)ol.p; a.lens_cap = n;
        a.d_names = on.p; a.names_cap = blob.size() - (c.which == 11); a.d_name_off = (uint64_t*)oo.p; a.off_cap = n + 1 - (c.which == 12);
        const int rc = rfq_select_rows(ctx, &in, &a, &g);
        char row[48]; snprintf(row, sizeof row, "first such row: %u)", c.row);
        if (rc != c.code) { fprintf(stderr, "%s: returned %d (%s), expected %d\n", c.what, rc, rfq_last_error(ctx), c.code); bad = 1; }
        else if (c.which <= 4 && !strstr(rfq_last_error(ctx), row)) { fprintf(stderr, "%s: the message names another row: %s\n", c.what, rfq_last_error(ctx)); bad = 1; }
        else if (c.code == RFQ_E_NOSPACE && !strstr(rfq_last_error(ctx), "need")) { fprintf(stderr, "%s: no \"need\" in: %s\n", c.what, rfq_last_error(ctx)); bad = 1; }
        else printf("%s: refused (%d) %s\n", c.what, rc, rfq_last_error(ctx));
        bad |= good(ctx);
    }
    return bad;
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = shapes(ctx);
    printf("shapes: %s\n", bad ? "FAILED" : "ok");
    bad |= refusals(ctx);
    rfq_destroy(ctx);
    printf("select_asan: %s\n", bad ? "FAILED" : "ok");
    return bad;
}
