// tag_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_select_rows with a tag (rfq_name_tag) on the SIMT-interpreter build (CPU only, no Python):
// tools/tag_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   tag_asan_main        good shapes of tests/_tag.py - the place (a space first, in the middle, last, twice, absent, a tab, names of 0 / 15 .. 17 / 255 .. 257 / 700
//   bytes, both places), the seams of the blob (a tag across a tile boundary, a head that ends on one, every alignment of the blob, many short names in a tile), parts
//   of 0 .. 32 bases at the starts 0 / 15 / 16 / 17 / lens - len with the last part the last bytes of an unaligned allocation, letters and codes, pairs with and without
//   a prefix - on the default formulation and on RFQ_TAG=general, into caller buffers of exactly the reported sizes (every allocation ends where its data ends),
//   compared with a host loop; then every refusal, each followed by a plain call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <string>
#include <vector>

struct Rows {
    uint32_t n = 0, L = 1; int codes = 0, pairs = 0; std::vector<uint8_t> B, Q, keep; std::vector<int32_t> lens, start, ts, tl; std::vector<std::string> names;
    std::string prefix; uint8_t sep = ':', join = '_', at = RFQ_TAG_AT_SPACE; bool has_keep = false, has_start = false, tagged = true;
};
static Rows make_rows(uint32_t n, uint32_t L, int codes) {
    Rows r; r.n = n; r.L = L; r.codes = codes; r.B.resize((size_t)n * L); r.Q.resize((size_t)n * L); r.lens.assign(n, (int32_t)L); r.names.resize(n); r.ts.assign(n, 0); r.tl.assign(n, 0);
    for (auto& x : r.B) x = codes ? (uint8_t)(rnd() % 5) : (uint8_t)"ACGTNacgtn"[rnd() % 10];
    for (auto& x : r.Q) x = (uint8_t)rnd();
    return r;
}
static std::string text(uint32_t i, uint32_t k) { std::string s(k, 'x'); for (uint32_t j = 0; j < k; j++) s[j] = (char)(33 + (i * 31 + j * 7) % 94); return s; }

// the host's names: X of the row's unit in its place
static std::string tagged(const Rows& r, uint32_t i) {
    if (!r.tagged) return r.names[i];
    auto part = [&](uint32_t row) { std::string p; for (int32_t k = 0; k < r.tl[row]; k++) { const uint8_t c = r.B[(size_t)row * r.L + r.ts[row] + k]; p += r.codes ? "ACGTN"[c] : (char)c; } return p; };
    std::string T;
    if (r.pairs) { const std::string a = part(i & ~1u), b = part(i | 1u); T = a + (a.size() && b.size() ? std::string(1, (char)r.join) : "") + b; } else T = part(i);
    const std::string X = T.empty() ? "" : std::string(1, (char)r.sep) + (r.prefix.empty() ? "" : r.prefix + (char)r.join) + T;
    const std::string& nm = r.names[i];
    size_t at = nm.size();
    if (r.at == RFQ_TAG_AT_SPACE) { const size_t sp = nm.find(' '); if (sp != std::string::npos) at = sp; }
    return nm.substr(0, at) + X + nm.substr(at);
}

// one size query and one call into exact buffers, against the host's own selection, on both formulations
static int run(rfq_ctx* ctx, const char* what, const Rows& r, uint32_t min_len, size_t in_shift, size_t out_shift) {
    const uint32_t n = r.n;
    std::vector<uint64_t> off(n + 1, 0); std::string blob;
    for (uint32_t i = 0; i < n; i++) { blob += r.names[i]; off[i + 1] = blob.size(); }
    std::vector<int> why(n, 0); std::vector<int64_t> st(n), ln(n);
    for (uint32_t i = 0; i < n; i++) { st[i] = r.has_start ? r.start[i] : 0; ln[i] = r.lens[i] - st[i]; why[i] = (r.has_keep && !r.keep[i]) ? 1 : (ln[i] < (int64_t)min_len ? 2 : 0); }
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; i++) { int w = why[i]; if (!w && r.pairs && why[i ^ 1]) w = 3; if (!w) idx.push_back(i); }
    const uint32_t m = (uint32_t)idx.size();
    std::string want; std::vector<uint64_t> woff(m + 1, 0); uint32_t ml = 0, mn = 0;
    for (uint32_t j = 0; j < m; j++) { const std::string t = tagged(r, idx[j]); want += t; woff[j + 1] = want.size(); if (t.size() > mn) mn = (uint32_t)t.size(); if (ln[idx[j]] > ml) ml = (uint32_t)ln[idx[j]]; }
    Dev db(ctx, r.B.data(), r.B.size(), in_shift), dq(ctx, r.Q.data(), r.Q.size(), in_shift), dl(ctx, r.lens.data(), n * 4ull);
    Dev dn(ctx, blob.data(), blob.size(), in_shift), dof(ctx, off.data(), off.size() * 8);
    Dev dk(ctx, r.keep.data(), r.has_keep ? n : 0), ds(ctx, r.start.data(), r.has_start ? n * 4ull : 0), dts(ctx, r.ts.data(), n * 4ull), dtl(ctx, r.tl.data(), n * 4ull);
    rfq_rows_in in = rows_in(n, r.L, r.codes, db, &dq, dl);
    in.d_names = dn.p; in.names_len = blob.size(); in.d_name_off = (const uint64_t*)dof.p;
    rfq_name_tag tg; memset(&tg, 0, sizeof tg);
    tg.d_tag_start = (const int32_t*)dts.p; tg.d_tag_len = (const int32_t*)dtl.p; tg.h_prefix = r.prefix.empty() ? nullptr : (const uint8_t*)r.prefix.data(); tg.prefix_len = (uint32_t)r.prefix.size();
    tg.sep = r.sep; tg.join = r.join; tg.at = r.at;
    std::vector<uint8_t> first;
    for (const char* opt : { (const char*)nullptr, "general" }) {
        if (!r.tagged && opt) break;
        rfq_set_option(ctx, "RFQ_TAG", opt);
        rfq_select_rows_args a; memset(&a, 0, sizeof a); rfq_select_rows_result q, g;
        a.d_keep = r.has_keep ? dk.p : nullptr; a.d_start = r.has_start ? (const int32_t*)ds.p : nullptr; a.pairs = r.pairs; a.min_len = min_len; a.tag = r.tagged ? &tg : nullptr;
        if (rfq_select_rows(ctx, &in, &a, &q)) { rfq_set_option(ctx, "RFQ_TAG", nullptr); return fail(what, rfq_last_error(ctx)); }
        if (q.n_rows != m || q.names_len != want.size() || q.max_len != ml || q.max_name != mn || q.n_in != n) { rfq_set_option(ctx, "RFQ_TAG", nullptr); return fail(what, "the size query disagrees with the host"); }
        const uint32_t L = (ml / 16 + 1) * 16; const size_t rb = (size_t)m * L;
        Dev ob(ctx, nullptr, rb, out_shift), ol(ctx, nullptr, m * 4ull), on(ctx, nullptr, want.size(), out_shift), oo(ctx, nullptr, (m + 1) * 8ull);
        a.row_len = L; a.pad_base = 0xA7; a.d_bases = ob.p; a.bases_cap = rb; a.d_lens = (int32_t*)ol.p; a.lens_cap = m;
        a.d_names = on.p; a.names_cap = want.size(); a.d_name_off = (uint64_t*)oo.p; a.off_cap = m + 1;
        const int rc = rfq_select_rows(ctx, &in, &a, &g);
        rfq_set_option(ctx, "RFQ_TAG", nullptr);
        if (rc) return fail(what, rfq_last_error(ctx));
        if (memcmp(&g, &q, sizeof g)) return fail(what, "the call's result differs from the size query's");
        std::vector<uint8_t> hb(rb + 1), hn(want.size() + 1); std::vector<uint64_t> ho(m + 1);
        rfq_copy_d2h(ctx, hb.data(), ob.p, rb); rfq_copy_d2h(ctx, hn.data(), on.p, want.size()); rfq_copy_d2h(ctx, ho.data(), oo.p, (m + 1) * 8ull);
        if (memcmp(hn.data(), want.data(), want.size())) {
            size_t k = 0; while (hn[k] == (uint8_t)want[k]) k++;
            fprintf(stderr, "%s (%s): the name blob differs at byte %zu of %zu\n", what, opt ? opt : "default", k, want.size()); return 1;
        }
        if (ho != woff) return fail(what, "the name offsets differ");
        for (uint32_t j = 0; j < m; j++) for (uint32_t k = 0; k < L; k++)
            if (hb[(size_t)j * L + k] != (k < ln[idx[j]] ? r.B[(size_t)idx[j] * r.L + st[idx[j]] + k] : 0xA7)) return fail(what, "a row byte differs");
        if (!opt) first = hn; else if (first != hn) return fail(what, "the formulations give different bytes");
    }
    return 0;
}

static int good(rfq_ctx* ctx) {
    Rows r = make_rows(70, 20, 0); r.tagged = false; r.pairs = 1;
    for (uint32_t i = 0; i < 70; i++) r.names[i] = text(i, 1 + i % 3);
    r.has_keep = true; r.keep.resize(70); for (uint32_t i = 0; i < 70; i++) r.keep[i] = i % 5 != 2;
    return run(ctx, "the plain call behind a refusal", r, 1, 0, 0);
}

static int shapes(rfq_ctx* ctx) {
    int bad = 0; char what[160];
    {   // 1: the place
        std::vector<std::string> nm = { " x", "ab cd", "abc ", "a b c", "abcd", "", "ab\tcd", " ", "\t", "a" };
        for (uint32_t k : { 15u, 16u, 17u, 255u, 256u, 257u, 700u }) {
            const std::string t = text(k, k);
            nm.push_back(t); nm.push_back(" " + t.substr(1)); nm.push_back(t.substr(0, k - 1) + " "); nm.push_back(t.substr(0, k / 2) + " " + t.substr(k / 2 + 1));
            nm.push_back(t.substr(0, 3) + " " + t.substr(4, k - 6) + " " + t.substr(k - 1)); nm.push_back(t.substr(0, k / 2) + "\t" + t.substr(k / 2 + 1));
        }
        Rows r = make_rows((uint32_t)nm.size(), 40, 0); r.names = nm; r.tl.assign(r.n, 8);
        for (uint8_t at : { (uint8_t)RFQ_TAG_AT_SPACE, (uint8_t)RFQ_TAG_AT_END }) for (size_t sh : { (size_t)0, (size_t)3, (size_t)15 }) {
            r.at = at; snprintf(what, sizeof what, "the place: at %u, shift %zu", at, sh);
            bad |= run(ctx, what, r, 1, sh, (sh * 3 + 1) % 16);
        }
        r.prefix = "UMI"; r.sep = '#'; r.has_keep = true; r.keep.resize(r.n); for (uint32_t i = 0; i < r.n; i++) r.keep[i] = i % 3 != 1;
        bad |= run(ctx, "the place: a prefix, rows dropped", r, 1, 0, 0);
    }
    {   // 2: the seams of the blob
        Rows r = make_rows(260, 24, 0);
        r.names[0] = text(0, 4090); r.names[1] = text(1, 4096 * 2 - 4099) + " rest of the name";
        for (uint32_t i = 2; i < r.n; i++) r.names[i] = text(i, 5 + i % 29) + (i % 3 ? " 1:N:0" : "");
        for (uint32_t i = 0; i < r.n; i++) { r.ts[i] = (int32_t)(i % 5); r.tl[i] = 8; }
        for (size_t sh = 0; sh < 16; sh++) {                                   // (tiles count from the 16-byte boundary below the blob: the first name shrinks with the shift, the seams stay on tile edges)
            r.names[0] = text(0, 4090 - (uint32_t)sh); snprintf(what, sizeof what, "blob seams: shift %zu", sh); bad |= run(ctx, what, r, 1, (sh * 7) % 16, sh);
        }
        Rows s = make_rows(700, 8, 0);
        for (uint32_t i = 0; i < s.n; i++) { s.names[i] = text(i, i % 4); s.ts[i] = (int32_t)(i % 4); s.tl[i] = i % 3 == 0 ? 0 : 1 + (int32_t)(i % 2); }
        bad |= run(ctx, "many names in a tile", s, 1, 0, 0); bad |= run(ctx, "many names in a tile, shifted", s, 1, 0, 5);
    }
    for (int codes = 0; codes < 2; codes++) {   // 3: the parts
        const int32_t lens_[] = { 0, 1, 15, 16, 17, 32 }, starts[] = { 0, 15, 16, 17, -1 };
        std::vector<int32_t> ts, tl;
        for (int32_t l : lens_) for (int32_t s : starts) { ts.push_back(s); tl.push_back(l); }
        ts.push_back(-1); tl.push_back(32);
        Rows r = make_rows((uint32_t)ts.size(), 50, codes);
        for (uint32_t i = 0; i < r.n; i++) { r.lens[i] = i + 1 == r.n ? 50 : 49 + (int32_t)(i & 1); r.tl[i] = tl[i]; r.ts[i] = ts[i] < 0 ? r.lens[i] - tl[i] : ts[i]; r.names[i] = text(i, 9 + i % 11) + " 2:N:0"; }
        r.has_start = true; r.start.resize(r.n); for (uint32_t i = 0; i < r.n; i++) r.start[i] = r.ts[i] + r.tl[i];
        for (size_t sh : { (size_t)0, (size_t)3 }) { snprintf(what, sizeof what, "parts: codes %d, shift %zu", codes, sh); bad |= run(ctx, what, r, 0, sh, sh); }
    }
    for (const char* prefix : { "", "UMI" }) {   // 4: pairs
        Rows r = make_rows(40, 36, 0); r.pairs = 1; r.prefix = prefix; r.join = prefix[0] ? '+' : '_';
        const int32_t pat[4][2] = { { 8, 6 }, { 8, 0 }, { 0, 6 }, { 0, 0 } };
        for (uint32_t i = 0; i < r.n; i++) { r.names[i] = text(i / 2, 12) + (i & 1 ? " 2:N:0" : " 1:N:0"); r.ts[i] = 2; r.tl[i] = pat[(i / 2) % 4][i & 1]; }
        r.has_keep = r.has_start = true; r.keep.assign(r.n, 1); r.start.assign(r.n, 10); r.keep[16] = 0; r.start[9] = 30;
        snprintf(what, sizeof what, "pairs: prefix \"%s\"", prefix);
        bad |= run(ctx, what, r, 10, 1, 2);
    }
    return bad;
}

static int refusals(rfq_ctx* ctx) {
    int bad = 0;
    const uint32_t n = 60, L = 24;
    Rows r = make_rows(n, L, 0);
    for (uint32_t i = 0; i < n; i++) r.names[i] = text(i, 4 + i % 9);
    std::vector<uint64_t> off(n + 1, 0); std::string blob;
    for (uint32_t i = 0; i < n; i++) { blob += r.names[i]; off[i + 1] = blob.size(); }
    const int32_t I32 = 0x7FFFFFFF;
    // which: 0 ts, 1 tl, 2 both (ts = lens - 3, tl = 4), 3 both = v, 4 a bad byte, 5 .. the host's; row2: a second offender behind the first (or 0); drop: keep[row] = 0
    struct Case { const char* what; int code; int which; uint32_t row, row2; int64_t v; bool drop; } cases[] = {
        { "tag_start = -1 in the last row", RFQ_E_ARG, 0, n - 1, 0, -1, false }, { "tag_start = -1 in a dropped row", RFQ_E_ARG, 0, 21, 0, -1, true },
        { "tag_len = -1 in the last row", RFQ_E_ARG, 1, n - 1, 0, -1, false }, { "tag_len = 33 in a dropped row", RFQ_E_ARG, 1, 33, 0, 33, true },
        { "tag_len = 33 twice", RFQ_E_ARG, 1, 7, 40, 33, false }, { "a part that ends behind its read, last row", RFQ_E_ARG, 2, n - 1, 0, 0, false },
        { "tag_start = tag_len = INT32_MAX", RFQ_E_ARG, 3, 31, 0, I32, true }, { "a bad part byte in the last row", RFQ_E_DATA, 4, n - 1, 0, 0, false },
        { "a bad part byte in a dropped row", RFQ_E_DATA, 4, 12, 0, 0, true }, { "0x20 as a part byte in the last row", RFQ_E_DATA, 4, n - 1, 0, 0x20, false },
        { "rows without names", RFQ_E_ARG, 5, 0, 0, 0, false }, { "null d_tag_start", RFQ_E_ARG, 6, 0, 0, 0, false }, { "null d_tag_len", RFQ_E_ARG, 7, 0, 0, 0, false },
        { "misaligned d_tag_start", RFQ_E_ARG, 8, 0, 0, 0, false }, { "misaligned d_tag_len", RFQ_E_ARG, 9, 0, 0, 0, false }, { "prefix_len = 15", RFQ_E_ARG, 10, 0, 0, 0, false },
        { "null h_prefix", RFQ_E_ARG, 11, 0, 0, 0, false }, { "sep = 0x20", RFQ_E_ARG, 12, 0, 0, 0, false }, { "join = 0x7f", RFQ_E_ARG, 13, 0, 0, 0, false },
        { "a tab in the prefix", RFQ_E_ARG, 14, 0, 0, 0, false }, { "at = 2", RFQ_E_ARG, 15, 0, 0, 0, false }, { "base_mode = 7", RFQ_E_ARG, 16, 0, 0, 0, false },
        { "null rows->d_bases", RFQ_E_ARG, 17, 0, 0, 0, false }, { "d_names on d_tag_start", RFQ_E_ARG, 18, 0, 0, 0, false }, { "d_lens on d_tag_len", RFQ_E_ARG, 19, 0, 0, 0, false },
        { "names_cap one short", RFQ_E_NOSPACE, 20, 0, 0, 0, false } };
    for (const Case& c : cases) for (int codes = 0; codes < 2; codes++) {
        std::vector<uint8_t> B = r.B, keep(n, 1); std::vector<int32_t> ts(n, 1), tl(n, 5);
        if (codes) for (auto& x : B) x = (uint8_t)(x % 5);
        for (uint32_t row : { c.row, c.row2 }) {
            if (c.which > 4 || (row == 0 && row != c.row)) continue;
            if (c.which == 0) ts[row] = (int32_t)c.v;
            if (c.which == 1) tl[row] = (int32_t)c.v;
            if (c.which == 2) { ts[row] = (int32_t)L - 3; tl[row] = 4; }
            if (c.which == 3) ts[row] = tl[row] = (int32_t)c.v;
            if (c.which == 4) B[(size_t)row * L + (c.v ? 1 : 5)] = c.v ? (uint8_t)c.v : 0xFF;
        }
        if (c.drop) keep[c.row] = 0;
        Dev db(ctx, B.data(), B.size(), 1), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, r.lens.data(), n * 4ull), dn(ctx, blob.data(), blob.size()), dof(ctx, off.data(), off.size() * 8);
        Dev dk(ctx, keep.data(), n), dts(ctx, ts.data(), n * 4ull), dtl(ctx, tl.data(), n * 4ull);
        const size_t nl = blob.size() + 6ull * n;
        Dev ol(ctx, nullptr, n * 4ull), on(ctx, nullptr, nl), oo(ctx, nullptr, (n + 1) * 8ull);
        rfq_rows_in in = rows_in(n, L, codes, db, &dq, dl);
        if (c.which == 16) in.base_mode = 7;
        if (c.which == 17) in.d_bases = nullptr;
        if (c.which != 5) { in.d_names = dn.p; in.names_len = blob.size(); in.d_name_off = (const uint64_t*)dof.p; }
        const uint8_t pre[16] = { 'A', '\t', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A' };
        rfq_name_tag tg; memset(&tg, 0, sizeof tg);
        tg.d_tag_start = c.which == 6 ? nullptr : (const int32_t*)(dts.p + (c.which == 8 ? 2 : 0)); tg.d_tag_len = c.which == 7 ? nullptr : (const int32_t*)(dtl.p + (c.which == 9 ? 1 : 0));
        tg.sep = c.which == 12 ? 0x20 : ':'; tg.join = c.which == 13 ? 0x7F : '_'; tg.at = c.which == 15 ? 2 : RFQ_TAG_AT_SPACE;
        if (c.which == 10) { tg.h_prefix = pre + 2; tg.prefix_len = 15; }
        if (c.which == 11) tg.prefix_len = 3;
        if (c.which == 14) { tg.h_prefix = pre; tg.prefix_len = 3; }
        rfq_select_rows_args a; memset(&a, 0, sizeof a); rfq_select_rows_result g;
        a.d_keep = dk.p; a.min_len = 1; a.tag = &tg; a.row_len = L;
        if (c.which != 5) { a.d_names = c.which == 18 ? dts.p + 4 : on.p; a.names_cap = c.which == 18 ? 16 : nl - (c.which == 20); a.d_name_off = (uint64_t*)oo.p; a.off_cap = n + 1; }
        a.d_lens = c.which == 19 ? (int32_t*)dtl.p : (int32_t*)ol.p; a.lens_cap = n;
        for (const char* opt : { (const char*)nullptr, "general" }) {
            rfq_set_option(ctx, "RFQ_TAG", opt);
            const int rc = rfq_select_rows(ctx, &in, &a, &g);
            rfq_set_option(ctx, "RFQ_TAG", nullptr);
            char row[48]; snprintf(row, sizeof row, "first such row: %u)", c.row2 && c.row2 < c.row ? c.row2 : c.row);
            if (rc != c.code) { fprintf(stderr, "%s: returned %d (%s), expected %d\n", c.what, rc, rfq_last_error(ctx), c.code); bad = 1; }
            else if (c.which <= 4 && !strstr(rfq_last_error(ctx), row)) { fprintf(stderr, "%s: the message names another row: %s\n", c.what, rfq_last_error(ctx)); bad = 1; }
            else if (c.code == RFQ_E_NOSPACE && !strstr(rfq_last_error(ctx), "need")) { fprintf(stderr, "%s: no \"need\" in: %s\n", c.what, rfq_last_error(ctx)); bad = 1; }
            else if (!codes && !opt) printf("%s: refused (%d) %s\n", c.what, rc, rfq_last_error(ctx));
        }
        bad |= good(ctx);
    }
    if (rfq_set_option(ctx, "RFQ_TAG", "staged") != RFQ_E_ARG) bad |= fail("RFQ_TAG=staged", "not refused");
    return bad;
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = shapes(ctx);
    printf("shapes: %s\n", bad ? "FAILED" : "ok");
    bad |= refusals(ctx);
    rfq_destroy(ctx);
    printf("%s\n", bad ? "FAILED" : "all ok");
    return bad ? 1 : 0;
}
