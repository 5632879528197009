// judge_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_judge_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/judge_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   judge_asan_main         the good shapes of tests/_judge.py - every step alone and all together over the row strides 1 .. 300 and 1500, 1 .. 2049 rows, buffer
//   shifts 0 / 1 / 7 / 15, both base modes, the default path and RFQ_JUDGE=general, each output alone and none - with rows in allocations that end where the rows
//   end and outputs of exactly n_rows entries, compared with a host reference written from include/rfq_hip.h; then every refusal, each followed by a good call.
//   Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <vector>

struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, Q; std::vector<int32_t> lens; };
// lengths 0 .. L, bases ACGTN (either case in ASCII mode) with G tails, scores that rise towards the middle of a read; noise behind the reads
static Rows make_rows(uint32_t n, uint32_t L, int codes) {
    Rows r; r.n = n; r.L = L; r.codes = codes; r.B.resize((size_t)n * L); r.Q.resize((size_t)n * L); r.lens.resize(n);
    static const char alpha[] = "ACGTACGTACGTACGTacgtNn";
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = i == 0 ? L : (i == n - 1 ? 0 : rnd() % (L + 1)), tail = rnd() % 3 ? 0 : rnd() % 9, ramp = 1 + rnd() % 7;
        r.lens[i] = (int32_t)l;
        for (uint32_t k = 0; k < L; k++) {
            uint8_t b = codes ? (uint8_t)(rnd() % 25 ? rnd() % 4 : 4) : (uint8_t)alpha[rnd() % 22];
            if (k + tail >= l) b = codes ? 2 : (rnd() % 5 ? 'G' : 'g');
            const uint32_t edge = k < l ? std::min(k, l - 1 - k) : 0;
            uint32_t q = 8 + edge * 30 / (ramp * 4) + rnd() % 19; q = q < 9 ? 0 : std::min(q - 9, 41u);
            if (rnd() % 97 == 0) q = 255;
            if (k >= l) { b = (uint8_t)rnd(); q = (uint8_t)rnd(); }
            r.B[(size_t)i * L + k] = b; r.Q[(size_t)i * L + k] = (uint8_t)q;
        }
    }
    return r;
}

struct Ref { std::vector<uint8_t> keep, why; std::vector<int32_t> start, len; std::vector<uint32_t> met; rfq_judge_rows_result s; };
static Ref reference(const Rows& r, const rfq_judge_rows_args& c) {
    Ref o; const uint32_t n = r.n; o.keep.resize(n); o.why.resize(n); o.start.resize(n); o.len.resize(n); o.met.resize(4ull * n); memset(&o.s, 0, sizeof o.s); o.s.n_rows = n;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* b = &r.B[(size_t)i * r.L]; const uint8_t* q = &r.Q[(size_t)i * r.L]; const int64_t l = r.lens[i];
        std::vector<int64_t> P(l + 1, 0);
        for (int64_t k = 0; k < l; k++) P[k + 1] = P[k] + q[k];
        auto isG = [&](uint8_t x) { return r.codes ? x == 2 : (x == 'G' || x == 'g'); };
        auto isN = [&](uint8_t x) { return r.codes ? x == 4 : (x == 'N' || x == 'n'); };
        int64_t a = std::min<int64_t>(c.trim_front, l), e = std::max<int64_t>(a, l - std::min<int64_t>(c.trim_tail, l));
        if (c.poly_g && e > a) { int64_t run = 0; while (e - 1 - run >= a && isG(b[e - 1 - run])) run++; if (run >= c.poly_g) e -= run; }
        const int64_t mq = c.cut_mean_q;
        if ((c.cut_flags & RFQ_CUT_FRONT) && e > a) { const int64_t w = std::min<int64_t>(c.cut_window, e - a); int64_t p = a; while (p <= e - w && P[p + w] - P[p] < mq * w) p++; if (p > e - w) e = a; else a = p; }
        if ((c.cut_flags & RFQ_CUT_RIGHT) && e > a) { const int64_t w = std::min<int64_t>(c.cut_window, e - a); int64_t p = a; while (p <= e - w && P[p + w] - P[p] >= mq * w) p++; if (p <= e - w) e = p; }
        if ((c.cut_flags & RFQ_CUT_TAIL) && e > a) { const int64_t w = std::min<int64_t>(c.cut_window, e - a); int64_t p = e - w; while (p >= a && P[p + w] - P[p] < mq * w) p--; if (p < a) e = a; else e = p + w; }
        if (c.max_len) e = std::min<int64_t>(e, a + c.max_len);
        const int64_t m = e - a, qsum = P[e] - P[a]; int64_t nc = 0, low = 0, tr = 0, q20 = 0, q30 = 0;
        for (int64_t k = a; k < e; k++) { nc += isN(b[k]); low += c.qual_q && q[k] < c.qual_q; tr += k + 1 < e && b[k] != b[k + 1]; q20 += q[k] >= 20; q30 += q[k] >= 30; }
        uint32_t why = 0;
        if (m < (int64_t)c.min_len) why |= RFQ_WHY_SHORT;
        if (c.max_n >= 0 && nc > c.max_n) why |= RFQ_WHY_N;
        if (qsum < (int64_t)c.min_mean_q * m) why |= RFQ_WHY_MEANQ;
        if (c.qual_q && low * 100 > (int64_t)c.max_lowq_pct * m) why |= RFQ_WHY_LOWQ;
        if (m > 1 && tr * 100 < (int64_t)c.min_complexity_pct * (m - 1)) why |= RFQ_WHY_COMPLEX;
        o.keep[i] = !why; o.why[i] = (uint8_t)why; o.start[i] = (int32_t)a; o.len[i] = (int32_t)m;
        o.met[4ull * i] = (uint32_t)qsum; o.met[4ull * i + 1] = (uint32_t)nc; o.met[4ull * i + 2] = (uint32_t)low; o.met[4ull * i + 3] = (uint32_t)tr;
        o.s.n_kept += !why; o.s.why_short += !!(why & 1); o.s.why_n += !!(why & 2); o.s.why_meanq += !!(why & 4); o.s.why_lowq += !!(why & 8); o.s.why_complex += !!(why & 16);
        o.s.bases_in += l; o.s.qsum_in += P[l];
        for (int64_t k = 0; k < l; k++) { o.s.q20_in += q[k] >= 20; o.s.q30_in += q[k] >= 30; }
        if (!why) { o.s.bases_out += m; o.s.qsum_out += qsum; o.s.q20_out += q20; o.s.q30_out += q30; }
    }
    return o;
}

static rfq_judge_rows_args crit() { rfq_judge_rows_args c; memset(&c, 0, sizeof c); c.max_n = -1; return c; }
static rfq_judge_rows_args filters(rfq_judge_rows_args c) { c.min_len = 20; c.max_n = 2; c.min_mean_q = 22; c.qual_q = 15; c.max_lowq_pct = 30; c.min_complexity_pct = 40; return c; }
static std::vector<rfq_judge_rows_args> steps() {
    std::vector<rfq_judge_rows_args> v; rfq_judge_rows_args c;
    c = crit(); c.trim_front = 3; c.trim_tail = 5; v.push_back(c);
    c = crit(); c.poly_g = 4; v.push_back(c);
    for (uint32_t f : { RFQ_CUT_FRONT, RFQ_CUT_RIGHT, RFQ_CUT_TAIL }) { c = crit(); c.cut_flags = f; c.cut_window = 4; c.cut_mean_q = 20; v.push_back(c); }
    c = crit(); c.max_len = 37; v.push_back(c);
    v.push_back(filters(crit()));
    c = filters(crit()); c.trim_front = 2; c.trim_tail = 1; c.poly_g = 5; c.cut_flags = 7; c.cut_window = 4; c.cut_mean_q = 17; c.max_len = 140; v.push_back(c);
    c = filters(crit()); c.cut_flags = 7; c.cut_window = 1000; c.cut_mean_q = 19; v.push_back(c);
    return v;
}

// outs: bits 1 keep, 2 start, 4 len, 8 why, 16 metrics
static int run(rfq_ctx* ctx, const char* what, const Rows& r, rfq_judge_rows_args c, int outs, size_t shift) {
    const uint32_t n = r.n; const Ref e = reference(r, c);
    Dev db(ctx, r.B.data(), r.B.size(), shift), dq(ctx, r.Q.data(), r.Q.size(), shift), dl(ctx, r.lens.data(), n * 4ull);
    Dev ok(ctx, nullptr, n), os(ctx, nullptr, n * 4ull), ol(ctx, nullptr, n * 4ull), ow(ctx, nullptr, n), om(ctx, nullptr, n * 16ull);
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, &dq, dl);
    c.d_keep = (outs & 1) ? ok.p : nullptr; c.d_start = (outs & 2) ? (int32_t*)os.p : nullptr; c.d_len = (outs & 4) ? (int32_t*)ol.p : nullptr;
    c.d_why = (outs & 8) ? ow.p : nullptr; c.d_metrics = (outs & 16) ? (uint32_t*)om.p : nullptr;
    rfq_judge_rows_result g;
    if (rfq_judge_rows(ctx, &in, &c, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e.s, sizeof g)) return fail(what, "the summary differs from the host's");
    if (!n) return 0;
    std::vector<uint8_t> hk(n + 1), hw(n + 1); std::vector<int32_t> hs(n + 1), hl(n + 1); std::vector<uint32_t> hm(4ull * n + 1);
    if (outs & 1) { rfq_copy_d2h(ctx, hk.data(), ok.p, n); if (memcmp(hk.data(), e.keep.data(), n)) return fail(what, "keep differs"); }
    if (outs & 2) { rfq_copy_d2h(ctx, hs.data(), os.p, n * 4ull); if (memcmp(hs.data(), e.start.data(), n * 4ull)) return fail(what, "start differs"); }
    if (outs & 4) { rfq_copy_d2h(ctx, hl.data(), ol.p, n * 4ull); if (memcmp(hl.data(), e.len.data(), n * 4ull)) return fail(what, "len differs"); }
    if (outs & 8) { rfq_copy_d2h(ctx, hw.data(), ow.p, n); if (memcmp(hw.data(), e.why.data(), n)) return fail(what, "why differs"); }
    if (outs & 16) { rfq_copy_d2h(ctx, hm.data(), om.p, n * 16ull); if (memcmp(hm.data(), e.met.data(), n * 16ull)) return fail(what, "metrics differ"); }
    return 0;
}

static int good(rfq_ctx* ctx) { const Rows r = make_rows(40, 33, 1); return run(ctx, "a good call after a refusal", r, steps()[7], 31, 0); }
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_judge_rows_args& c, const char* needle) {
    rfq_judge_rows_result g;
    const int rc = rfq_judge_rows(ctx, &in, &c, &g);
    if (rc != RFQ_E_ARG) return fail(what, "not refused with RFQ_E_ARG");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0;
    const std::vector<rfq_judge_rows_args> S = steps();
    const uint32_t lens[] = { 1, 15, 16, 17, 100, 150, 160, 255, 256, 257, 300, 1500 }, rows[] = { 1, 2, 255, 257, 2049 }; const size_t shifts[] = { 0, 1, 7, 15 };
    for (int general = 0; general < 2 && !bad; general++) {
        if (rfq_set_option(ctx, "RFQ_JUDGE", general ? "general" : nullptr)) return fail("RFQ_JUDGE", rfq_last_error(ctx));
        uint32_t k = 0;
        for (uint32_t L : lens) for (size_t si = 0; si < S.size() && !bad; si++, k++) {
            const uint32_t n = L == 1500 ? 5 : ((si == 7) ? rows[(k / 9) % 5] : rows[k % 4]);
            const Rows r = make_rows(n, L, (int)(k & 1));
            char what[128]; snprintf(what, sizeof what, "general %d row_len %u step %zu rows %u shift %zu", general, L, si, n, shifts[k % 4]);
            bad |= run(ctx, what, r, S[si], 31, shifts[k % 4]); calls++;
        }
        const Rows r = make_rows(300, 150, 0);
        for (int outs : { 1, 2, 4, 8, 16, 0 }) { bad |= run(ctx, "one output alone", r, S[7], outs, 3); calls++; }
    }
    rfq_set_option(ctx, "RFQ_JUDGE", nullptr);
    {   // long rows on the default path, and no rows at all
        const Rows r = make_rows(3, 70000, 1);
        bad |= run(ctx, "rows of 70000", r, S[7], 31, 5); bad |= run(ctx, "rows of 70000, a window of 1000", r, S[8], 31, 0); calls += 2;
        const Rows z = make_rows(0, 16, 0); bad |= run(ctx, "no rows", z, S[7], 31, 0); calls++;
    }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 32, 0);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);                   // (a word more: the misaligned d_lens stays inside it)
        Dev db(ctx, r.B.data(), r.B.size()), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, lp.data(), 160 + 4), out(ctx, nullptr, 4096);
        const rfq_rows_in in = rows_in(40, 32, 0, db, &dq, dl);
        rfq_judge_rows_args c; rfq_rows_in x;
        c = crit(); c.cut_flags = 8; c.cut_window = 4; bad |= refused(ctx, "unknown cut_flags bits", in, c, "cut_flags");
        c = crit(); c.cut_flags = 1; bad |= refused(ctx, "cut_window 0", in, c, "cut_window");
        c = crit(); c.cut_flags = 4; c.cut_window = 1001; bad |= refused(ctx, "cut_window 1001", in, c, "cut_window");
        c = crit(); c.qual_q = 5; c.max_lowq_pct = 101; bad |= refused(ctx, "max_lowq_pct 101", in, c, "percentage");
        c = crit(); c.min_complexity_pct = 101; bad |= refused(ctx, "min_complexity_pct 101", in, c, "percentage");
        c = crit(); x = in; x.base_mode = 2; bad |= refused(ctx, "bad base_mode", x, c, "base_mode");
        x = in; x.row_len = 0; bad |= refused(ctx, "row_len 0", x, c, "row_len");
        x = in; x.d_quals = nullptr;
        c = crit(); c.cut_flags = 2; c.cut_window = 4; bad |= refused(ctx, "no quals with a cut flag", x, c, "d_quals");
        c = crit(); c.min_mean_q = 1; bad |= refused(ctx, "no quals with min_mean_q", x, c, "d_quals");
        c = crit(); c.qual_q = 1; bad |= refused(ctx, "no quals with qual_q", x, c, "d_quals");
        x = in; x.d_bases = nullptr;
        c = crit(); c.poly_g = 3; bad |= refused(ctx, "no bases with poly_g", x, c, "d_bases");
        c = crit(); c.max_n = 0; bad |= refused(ctx, "no bases with max_n", x, c, "d_bases");
        c = crit(); c.min_complexity_pct = 1; bad |= refused(ctx, "no bases with min_complexity_pct", x, c, "d_bases");
        c = crit(); x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= refused(ctx, "misaligned d_lens", x, c, "aligned");
        c = crit(); c.d_start = (int32_t*)(out.p + 1); bad |= refused(ctx, "misaligned d_start", in, c, "aligned");
        c = crit(); c.d_len = (int32_t*)(out.p + 2); bad |= refused(ctx, "misaligned d_len", in, c, "aligned");
        c = crit(); c.d_metrics = (uint32_t*)(out.p + 3); bad |= refused(ctx, "misaligned d_metrics", in, c, "aligned");
        c = crit(); c.d_keep = db.p + 40 * 32 - 1; bad |= refused(ctx, "keep on bases", in, c, "overlaps");
        c = crit(); c.d_why = dq.p - 39; bad |= refused(ctx, "why ends in quals", in, c, "overlaps");
        c = crit(); c.d_start = (int32_t*)dl.p; bad |= refused(ctx, "start on lens", in, c, "overlaps");
        c = crit(); c.d_metrics = (uint32_t*)(dq.p + 16); bad |= refused(ctx, "metrics on quals", in, c, "overlaps");
        for (int general = 0; general < 2; general++) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 20u, 39u }) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 160); x = in; x.d_lens = (const int32_t*)d2.p;
            c = S[7]; c.d_keep = out.p; c.d_start = (int32_t*)(out.p + 64); c.d_metrics = (uint32_t*)(out.p + 1024);
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_JUDGE", general ? "general" : nullptr);
            rfq_judge_rows_result g;
            if (rfq_judge_rows(ctx, &x, &c, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_JUDGE", nullptr);
            bad |= good(ctx);
        }
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("judge_asan: %d good calls (12 row strides x 9 criteria sets x 2 paths, outputs alone, rows of 70000, no rows), 21 host and 12 device refusals each followed by a good call: all as the host reference says, no sanitizer report\n", calls);
    return 0;
}
