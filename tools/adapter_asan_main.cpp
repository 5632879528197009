// adapter_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_adapter_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/adapter_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   adapter_asan_main       the good shapes of tests/_adapter.py - overlap only, adapters only and both over the row strides 1 .. 1100, 1 .. 129 pairs, buffer shifts
//   0 / 1 / 7 / 15, both base modes, the default path and RFQ_ADAPTER=general, each output alone and none - with rows in allocations that end where the rows end
//   and outputs of exactly their size, compared with a host loop written from include/rfq_hip.h; then every refusal, each followed by a good call.
//   Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <string>
#include <vector>

static const char AD1[] = "AGATCGGAAGAGC", AD2[] = "CTGTCTCTTATAC";
struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B; std::vector<int32_t> lens; };
static uint8_t base_of(uint32_t cls, int codes) { return codes ? (uint8_t)cls : (uint8_t)("ACGTacgt"[cls + (rnd() % 4 ? 0 : 4)]); }
static uint32_t cls_of(uint8_t b, int codes) {
    if (codes) return b < 4 ? b : 4;
    switch (b) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}
// pairs at stride L: lengths 0 .. L, bases with a few others among them; every third pair comes from a fragment with the adapters behind it; noise behind the reads
static Rows make_rows(uint32_t pairs, uint32_t L, int codes) {
    Rows r; r.n = 2 * pairs; r.L = L; r.codes = codes; r.B.resize((size_t)r.n * L); r.lens.resize(r.n);
    for (uint32_t k = 0; k < pairs; k++) {
        uint32_t l1 = k == 0 ? L : rnd() % (L + 1), l2 = k == pairs - 1 ? 0 : rnd() % (L + 1);
        std::vector<uint8_t> r1(L), r2(L);
        for (uint32_t j = 0; j < L; j++) { r1[j] = rnd() % 31 ? base_of(rnd() % 4, codes) : (codes ? (uint8_t)(4 + rnd() % 252) : (uint8_t)"NnRY"[rnd() % 4]);
                                           r2[j] = rnd() % 31 ? base_of(rnd() % 4, codes) : (codes ? (uint8_t)(4 + rnd() % 252) : (uint8_t)"NnRY"[rnd() % 4]); }
        if (k % 3 == 1) {
            l1 = L / 2 + rnd() % (L - L / 2 + 1); l2 = l1 - std::min(l1, rnd() % 3);
            const uint32_t choice[] = { l1 / 3 + 1, l1 ? l1 - 1 : 1, l1 + 1, l1 + l1 / 2 + 1 }, ins = choice[rnd() % 4];
            std::vector<uint32_t> f(ins);
            for (auto& x : f) x = rnd() % 4;
            for (uint32_t j = 0; j < L; j++) {
                if (j < ins) { r1[j] = base_of(f[j], codes); r2[j] = base_of(3 - f[ins - 1 - j], codes); }
                else if (j < ins + 13) { r1[j] = base_of(cls_of((uint8_t)AD1[j - ins], 0), codes); r2[j] = base_of(cls_of((uint8_t)AD2[j - ins], 0), codes); }
                else { r1[j] = (uint8_t)rnd(); r2[j] = (uint8_t)rnd(); }
            }
        }
        for (uint32_t j = 0; j < L; j++) { if (j >= l1) r1[j] = (uint8_t)rnd(); if (j >= l2) r2[j] = (uint8_t)rnd(); }
        memcpy(&r.B[(size_t)(2 * k) * L], r1.data(), L); memcpy(&r.B[(size_t)(2 * k + 1) * L], r2.data(), L);
        r.lens[2 * k] = (int32_t)l1; r.lens[2 * k + 1] = (int32_t)l2;
    }
    return r;
}

struct Ref { std::vector<int32_t> len, insert, diff; std::vector<uint8_t> how; std::vector<uint64_t> hist; rfq_adapter_rows_result s; };
// the rules of include/rfq_hip.h as plain loops
static Ref reference(const Rows& r, const rfq_adapter_rows_args& c) {
    Ref o; const uint32_t n = r.n, np = c.pairs ? n / 2 : 0; o.len.resize(n); o.how.resize(n); o.insert.assign(np, -1); o.diff.assign(np, 0); o.hist.assign(c.hist_len, 0);
    memset(&o.s, 0, sizeof o.s); o.s.n_rows = n; o.s.n_pairs = np;
    std::vector<int64_t> cut_o(n);
    for (uint32_t i = 0; i < n; i++) cut_o[i] = r.lens[i];
    for (uint32_t k = 0; k < np; k++) {
        const uint8_t* x = &r.B[(size_t)(2 * k) * r.L]; const uint8_t* z = x + r.L; const int64_t l1 = r.lens[2 * k], l2 = r.lens[2 * k + 1], mo = c.min_overlap;
        auto test = [&](int64_t d) {
            const int64_t lo = std::max<int64_t>(0, -d), hi = std::min(l2, l1 - d), ov = hi - lo; int64_t diff = 0;
            if (ov < mo || ov <= 0) return false;
            for (int64_t j = lo; j < hi; j++) { const uint32_t a = cls_of(x[j + d], r.codes), b = cls_of(z[l2 - 1 - j], r.codes); diff += !(a < 4 && b < 4 && a == 3 - b); }
            if (diff > (int64_t)c.max_diff || diff * 100 > (int64_t)c.max_diff_pct * ov) return false;
            o.insert[k] = (int32_t)(d + l2); o.diff[k] = (int32_t)diff;
            return true;
        };
        bool found = false;
        for (int64_t d = 0; d <= l1 - mo && !found; d++) found = test(d);
        for (int64_t d = -1; d >= -(l2 - mo) && !found; d--) found = test(d);
        if (found) {
            o.s.pairs_found++; cut_o[2 * k] = std::min<int64_t>(l1, o.insert[k]); cut_o[2 * k + 1] = std::min<int64_t>(l2, o.insert[k]);
            if (c.hist_len) o.hist[std::min<uint32_t>((uint32_t)o.insert[k], c.hist_len - 1)]++;
        }
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* x = &r.B[(size_t)i * r.L]; const int64_t l = r.lens[i];
        const uint8_t* A = (c.pairs && (i & 1)) ? c.h_adapter2 : c.h_adapter1; const int64_t m = A ? ((c.pairs && (i & 1)) ? c.adapter2_len : c.adapter1_len) : 0;
        int64_t cut_a = l;
        for (int64_t p = 0; m && p < l; p++) {
            const int64_t cc = std::min(m, l - p); int64_t diff = 0;
            for (int64_t j = 0; j < cc; j++) diff += cls_of(x[p + j], r.codes) != cls_of(A[j], 0);
            if (cc >= (int64_t)c.adapter_min && (c.adapter_mm_per ? diff * c.adapter_mm_per <= cc : diff == 0)) { cut_a = p; break; }
        }
        const int64_t len = std::min(cut_o[i], cut_a); const uint32_t how = (cut_o[i] < l ? 1u : 0u) | (cut_a < l ? 2u : 0u);
        o.len[i] = (int32_t)len; o.how[i] = (uint8_t)how;
        o.s.rows_cut += how != 0; o.s.rows_cut_overlap += how & 1; o.s.rows_cut_adapter += how >> 1; o.s.bases_in += l; o.s.bases_out += len;
    }
    return o;
}

static rfq_adapter_rows_args crit(int which, uint32_t L) {
    rfq_adapter_rows_args c; memset(&c, 0, sizeof c);
    if (which != 1) { c.pairs = 1; c.min_overlap = L < 64 ? 4 : 12; c.max_diff = 3; c.max_diff_pct = 20; }
    if (which != 0) { c.h_adapter1 = (const uint8_t*)AD1; c.adapter1_len = 13; c.adapter_min = 4; c.adapter_mm_per = 6; }
    if (which == 2) { c.h_adapter2 = (const uint8_t*)AD2; c.adapter2_len = 13; c.hist_len = std::min(2 * L, 300u) + 1; }
    return c;
}

// outs: bits 1 len, 2 how, 4 insert, 8 diff, 16 hist
static int run(rfq_ctx* ctx, const char* what, const Rows& r, rfq_adapter_rows_args c, int outs, size_t shift) {
    const uint32_t n = r.n, np = n / 2; const Ref e = reference(r, c);
    if (!c.pairs) outs &= 3;
    if (!c.hist_len) outs &= ~16;
    Dev db(ctx, r.B.data(), r.B.size(), shift), dl(ctx, r.lens.data(), n * 4ull);
    Dev ol(ctx, nullptr, n * 4ull), oh(ctx, nullptr, n), oi(ctx, nullptr, np * 4ull), od(ctx, nullptr, np * 4ull), oH(ctx, nullptr, c.hist_len * 8ull);
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, nullptr, dl);
    c.d_len = (outs & 1) ? (int32_t*)ol.p : nullptr; c.d_how = (outs & 2) ? oh.p : nullptr; c.d_insert = (outs & 4) ? (int32_t*)oi.p : nullptr;
    c.d_diff = (outs & 8) ? (int32_t*)od.p : nullptr; c.d_insert_hist = (outs & 16) ? (uint64_t*)oH.p : nullptr;
    rfq_adapter_rows_result g;
    if (rfq_adapter_rows(ctx, &in, &c, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e.s, sizeof g)) return fail(what, "the summary differs from the host's");
    std::vector<uint8_t> hh(n + 1); std::vector<int32_t> hl(n + 1), hi(np + 1), hd(np + 1); std::vector<uint64_t> hH(c.hist_len + 1);
    if (n && (outs & 1)) { rfq_copy_d2h(ctx, hl.data(), ol.p, n * 4ull); if (memcmp(hl.data(), e.len.data(), n * 4ull)) return fail(what, "len differs"); }
    if (n && (outs & 2)) { rfq_copy_d2h(ctx, hh.data(), oh.p, n); if (memcmp(hh.data(), e.how.data(), n)) return fail(what, "how differs"); }
    if (np && (outs & 4)) { rfq_copy_d2h(ctx, hi.data(), oi.p, np * 4ull); if (memcmp(hi.data(), e.insert.data(), np * 4ull)) return fail(what, "insert differs"); }
    if (np && (outs & 8)) { rfq_copy_d2h(ctx, hd.data(), od.p, np * 4ull); if (memcmp(hd.data(), e.diff.data(), np * 4ull)) return fail(what, "diff differs"); }
    if (outs & 16) { rfq_copy_d2h(ctx, hH.data(), oH.p, c.hist_len * 8ull); if (memcmp(hH.data(), e.hist.data(), c.hist_len * 8ull)) return fail(what, "the histogram differs"); }
    return 0;
}

static int good(rfq_ctx* ctx) { const Rows r = make_rows(20, 33, 1); return run(ctx, "a good call after a refusal", r, crit(2, 33), 31, 0); }
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_adapter_rows_args& c, const char* needle) {
    rfq_adapter_rows_result g;
    const int rc = rfq_adapter_rows(ctx, &in, &c, &g);
    if (rc != RFQ_E_ARG) return fail(what, "not refused with RFQ_E_ARG");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, host_refusals = 0, device_refusals = 0;
    const uint32_t strides[] = { 1, 15, 16, 17, 63, 64, 65, 100, 150, 160, 255, 256, 257, 300, 1024, 1100 }, pairs[] = { 1, 2, 127, 129 }; const size_t shifts[] = { 0, 1, 7, 15 };
    for (int general = 0; general < 2 && !bad; general++) {
        if (rfq_set_option(ctx, "RFQ_ADAPTER", general ? "general" : nullptr)) return fail("RFQ_ADAPTER", rfq_last_error(ctx));
        uint32_t k = 0;
        for (uint32_t L : strides) for (int which = 0; which < 3 && !bad; which++, k++) {
            const uint32_t cap = L >= 1024 ? 5 : (L >= 255 ? 33 : 129), np = std::min(pairs[k % 4], cap);
            const Rows r = make_rows(np, L, (int)(k & 1));
            char what[128]; snprintf(what, sizeof what, "general %d row_len %u criteria %d pairs %u shift %zu", general, L, which, np, shifts[k % 4]);
            bad |= run(ctx, what, r, crit(which, L), 31, shifts[k % 4]); calls++;
        }
        const Rows r = make_rows(100, 150, 0);
        for (int outs : { 1, 2, 4, 8, 16, 0 }) { bad |= run(ctx, "one output alone", r, crit(2, 150), outs, 3); calls++; }
        rfq_adapter_rows_args c = crit(2, 150);
        for (uint32_t hl : { 1u, 2u, 400u, 65536u }) { c.hist_len = hl; bad |= run(ctx, "histogram lengths", r, c, 16, 9); calls++; }
    }
    rfq_set_option(ctx, "RFQ_ADAPTER", nullptr);
    { const Rows z = make_rows(0, 16, 0); bad |= run(ctx, "no rows", z, crit(2, 16), 31, 0); calls++; }
    if (!bad) {   // the refusals
        const Rows r = make_rows(20, 32, 0);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);                   // (a word more: the misaligned d_lens stays inside it)
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, lp.data(), 160 + 4), out(ctx, nullptr, 8192);
        const rfq_rows_in in = rows_in(40, 32, 0, db, nullptr, dl);
        const rfq_adapter_rows_args both = crit(2, 32); rfq_adapter_rows_args single = crit(1, 32), c; rfq_rows_in x;
        const std::string long_ad(65, 'A');
#define REFUSED(WHAT, IN, C, NEEDLE) { bad |= refused(ctx, WHAT, IN, C, NEEDLE); host_refusals++; }
        x = in; x.n_rows = 39; REFUSED("odd n_rows with pairs", x, both, "pairs")
        c = both; c.min_overlap = 0; REFUSED("min_overlap 0", in, c, "min_overlap")
        c = both; c.max_diff_pct = 101; REFUSED("max_diff_pct 101", in, c, "max_diff_pct")
        c = both; c.h_adapter1 = (const uint8_t*)long_ad.data(); c.adapter1_len = 65; REFUSED("an adapter of 65", in, c, "at most 64")
        c = both; c.h_adapter2 = (const uint8_t*)"ACGNT"; c.adapter2_len = 5; REFUSED("an adapter with N", in, c, "ACGTacgt")
        c = single; c.h_adapter2 = (const uint8_t*)AD2; c.adapter2_len = 13; REFUSED("adapter 2 without pairs", in, c, "for pairs")
        c = single; c.d_insert = (int32_t*)out.p; REFUSED("d_insert without pairs", in, c, "for pairs")
        c = single; c.d_diff = (int32_t*)out.p; REFUSED("d_diff without pairs", in, c, "for pairs")
        c = single; c.hist_len = 4; c.d_insert_hist = (uint64_t*)out.p; REFUSED("d_insert_hist without pairs", in, c, "for pairs")
        c = single; c.adapter_min = 0; REFUSED("adapter_min 0", in, c, "adapter_min")
        c = single; c.adapter_min = 65; REFUSED("adapter_min 65", in, c, "adapter_min")
        c = both; c.hist_len = 0; c.d_insert_hist = (uint64_t*)out.p; REFUSED("hist_len 0 with a histogram", in, c, "hist_len")
        c = both; c.hist_len = 65537; REFUSED("hist_len 65537", in, c, "hist_len")
        x = in; x.d_bases = nullptr; REFUSED("no bases", x, both, "d_bases")
        x = in; x.row_len = 0; REFUSED("row_len 0", x, both, "row_len")
        x = in; x.base_mode = 2; REFUSED("bad base_mode", x, both, "base_mode")
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); REFUSED("misaligned d_lens", x, both, "aligned")
        c = both; c.d_len = (int32_t*)(out.p + 2); REFUSED("misaligned d_len", in, c, "aligned")
        c = both; c.d_insert = (int32_t*)(out.p + 1); REFUSED("misaligned d_insert", in, c, "aligned")
        c = both; c.d_diff = (int32_t*)(out.p + 3); REFUSED("misaligned d_diff", in, c, "aligned")
        c = both; c.d_insert_hist = (uint64_t*)(out.p + 4); REFUSED("misaligned d_insert_hist", in, c, "aligned")
        c = both; c.d_len = (int32_t*)dl.p; REFUSED("len on lens", in, c, "overlaps")
        c = both; c.d_how = db.p + 40 * 32 - 1; REFUSED("how on the last base", in, c, "overlaps")
        c = both; c.d_diff = (int32_t*)(dl.p + 4 * 39); REFUSED("diff on the last length", in, c, "overlaps")
        c = both; c.d_insert_hist = (uint64_t*)(db.p + 16); REFUSED("hist on bases", in, c, "overlaps")
#undef REFUSED
        for (int general = 0; general < 2; general++) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 21u, 39u }) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 160); x = in; x.d_lens = (const int32_t*)d2.p;
            c = both; c.d_len = (int32_t*)out.p; c.d_insert = (int32_t*)(out.p + 1024); c.d_insert_hist = (uint64_t*)(out.p + 4096);
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_ADAPTER", general ? "general" : nullptr);
            rfq_adapter_rows_result g;
            if (rfq_adapter_rows(ctx, &x, &c, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_ADAPTER", nullptr);
            bad |= good(ctx); device_refusals++;
        }
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("adapter_asan: %d good calls (16 row strides x 3 criteria sets x 2 paths, outputs alone, histogram lengths, no rows), %d host and %d device refusals each followed by a good call: "
           "all as the host loop says, no sanitizer report\n", calls, host_refusals, device_refusals);
    return 0;
}
