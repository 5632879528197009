// dedup_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_dedup_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/dedup_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   dedup_asan_main         the good shapes of tests/_dedup.py - planted classes over the row strides 1 .. 1500, rows and pairs, both modes, a key_len, a candidate
//   mask, buffer shifts 0 / 1 / 7 / 15, the default table and RFQ_DEDUP=collide, each output alone and none - with rows in allocations that end where the rows end
//   and outputs of exactly the entries a call may write, compared with a host reference (a std::map from key bytes to members) written from include/rfq_hip.h;
//   then every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <map>
#include <string>
#include <vector>

struct Rows { uint32_t n = 0, L = 1; std::vector<uint8_t> B, Q, cand; std::vector<int32_t> lens; };
// n rows (nr to a unit) in about n / 4 classes of uneven sizes: a class has its own lengths and bytes, a member its own noise behind its reads and its own scores
static Rows make_rows(uint32_t n, uint32_t L, uint32_t nr, bool mask) {
    Rows r; r.n = n; r.L = L; r.B.resize((size_t)n * L); r.Q.resize((size_t)n * L); r.lens.resize(n); if (mask) r.cand.resize(n);
    const uint32_t U = n / nr, nc = std::min(200u, U / 4 + 1);
    std::vector<uint8_t> cb((size_t)nc * nr * L); std::vector<uint32_t> cl(nc * nr);
    static const char alpha[] = "ACGTacgtNn";
    for (auto& b : cb) b = (uint8_t)alpha[rnd() % 10];
    for (uint32_t i = 0; i < nc * nr; i++) cl[i] = i < 2 * nr ? L : rnd() % (L + 1);
    for (uint32_t u = 0; u < U; u++) {
        const uint32_t c = rnd() % 3 ? rnd() % std::min(nc, 4u) : rnd() % nc;             // (a few large classes, many small ones)
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * u + i, l = cl[c * nr + i]; r.lens[g] = (int32_t)l;
            for (uint32_t k = 0; k < L; k++) { r.B[(size_t)g * L + k] = k < l ? cb[((size_t)c * nr + i) * L + k] : (uint8_t)rnd(); r.Q[(size_t)g * L + k] = (uint8_t)(rnd() % 42); }
            if (mask) r.cand[g] = rnd() % 5 ? (uint8_t)(1 + rnd() % 255) : 0;
        }
    }
    return r;
}

struct Ref { std::vector<uint8_t> keep; std::vector<int32_t> dup_of; std::vector<uint32_t> count; std::vector<uint64_t> hist; rfq_dedup_rows_result s; };
static Ref reference(const Rows& r, const rfq_dedup_rows_args& a) {
    const uint32_t nr = a.pairs ? 2 : 1, U = r.n / nr;
    Ref o; o.keep.assign(r.n, 0); o.dup_of.assign(U, -1); o.count.assign(U, 0); o.hist.assign(a.hist_len, 0); memset(&o.s, 0, sizeof o.s); o.s.n_units = U;
    std::map<std::string, std::vector<uint32_t>> classes; std::vector<uint64_t> score(U, 0), bases(U, 0);
    for (uint32_t u = 0; u < U; u++) {
        bool cand = true; std::string key;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * u + i, l = (uint32_t)r.lens[g], k = a.key_len && a.key_len < l ? a.key_len : l;
            if (!r.cand.empty() && !r.cand[g]) cand = false;
            key.append((const char*)&k, 4); key.append((const char*)&r.B[(size_t)g * r.L], k);
            for (uint32_t j = 0; j < k; j++) score[u] += r.Q[(size_t)g * r.L + j];
            bases[u] += l;
        }
        if (!cand) continue;
        o.s.n_candidates++; o.s.bases_in += bases[u];
        classes[key].push_back(u);
    }
    for (auto& kv : classes) {
        const std::vector<uint32_t>& m = kv.second; uint32_t rep = m[0];
        if (a.mode == RFQ_DEDUP_BEST_QUAL) for (uint32_t u : m) if (score[u] > score[rep]) rep = u;      // (ascending: the first of the best stays)
        for (uint32_t u : m) o.dup_of[u] = (int32_t)rep;
        o.count[rep] = (uint32_t)m.size();
        for (uint32_t i = 0; i < nr; i++) o.keep[nr * rep + i] = 1;
        o.s.n_classes++; o.s.bases_kept += bases[rep]; o.s.max_class = std::max<uint64_t>(o.s.max_class, m.size());
        if (a.hist_len) o.hist[std::min<size_t>(m.size(), a.hist_len) - 1]++;
    }
    o.s.n_dups = o.s.n_candidates - o.s.n_classes;
    return o;
}

// outs: bits 1 keep, 2 dup_of, 4 count, 8 hist
static int run(rfq_ctx* ctx, const char* what, const Rows& r, rfq_dedup_rows_args a, int outs, size_t shift, bool quals = true) {
    const uint32_t n = r.n, U = n / (a.pairs ? 2 : 1); const Ref e = reference(r, a);
    Dev db(ctx, r.B.data(), r.B.size(), shift), dq(ctx, r.Q.data(), r.Q.size(), shift), dl(ctx, r.lens.data(), n * 4ull), dc(ctx, r.cand.data(), r.cand.size());
    Dev ok(ctx, nullptr, n), od(ctx, nullptr, U * 4ull), oc(ctx, nullptr, U * 4ull), oh(ctx, nullptr, a.hist_len * 8ull);
    const rfq_rows_in in = rows_in(n, r.L, 0, db, quals ? &dq : nullptr, dl);
    a.d_in = r.cand.empty() ? nullptr : dc.p;
    a.d_keep = (outs & 1) ? ok.p : nullptr; a.d_dup_of = (outs & 2) ? (int32_t*)od.p : nullptr; a.d_count = (outs & 4) ? (uint32_t*)oc.p : nullptr;
    a.d_hist = (outs & 8) && a.hist_len ? (uint64_t*)oh.p : nullptr;
    rfq_dedup_rows_result g;
    if (rfq_dedup_rows(ctx, &in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e.s, sizeof g)) return fail(what, "the summary differs from the host's");
    std::vector<uint8_t> hk(n + 1); std::vector<int32_t> hd(U + 1); std::vector<uint32_t> hc(U + 1); std::vector<uint64_t> hh(a.hist_len + 1);
    if ((outs & 1) && n) { rfq_copy_d2h(ctx, hk.data(), ok.p, n); if (memcmp(hk.data(), e.keep.data(), n)) return fail(what, "keep differs"); }
    if ((outs & 2) && U) { rfq_copy_d2h(ctx, hd.data(), od.p, U * 4ull); if (memcmp(hd.data(), e.dup_of.data(), U * 4ull)) return fail(what, "dup_of differs"); }
    if ((outs & 4) && U) { rfq_copy_d2h(ctx, hc.data(), oc.p, U * 4ull); if (memcmp(hc.data(), e.count.data(), U * 4ull)) return fail(what, "count differs"); }
    if (a.d_hist) { rfq_copy_d2h(ctx, hh.data(), oh.p, a.hist_len * 8ull); if (memcmp(hh.data(), e.hist.data(), a.hist_len * 8ull)) return fail(what, "the histogram differs"); }
    return 0;
}

static rfq_dedup_rows_args args(int pairs, int mode, uint32_t key_len, uint32_t hist_len) {
    rfq_dedup_rows_args a; memset(&a, 0, sizeof a); a.pairs = pairs; a.mode = mode; a.key_len = key_len; a.hist_len = hist_len; return a;
}
static int good(rfq_ctx* ctx) { const Rows r = make_rows(60, 33, 2, true); return run(ctx, "a good call after a refusal", r, args(1, RFQ_DEDUP_BEST_QUAL, 0, 4), 15, 0); }
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_dedup_rows_args& a, const char* needle) {
    rfq_dedup_rows_result g;
    const int rc = rfq_dedup_rows(ctx, &in, &a, &g);
    if (rc != RFQ_E_ARG) return fail(what, "not refused with RFQ_E_ARG");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, refusals = 0;
    const uint32_t lens[] = { 1, 15, 16, 17, 100, 150, 256, 257, 300, 1024, 1025, 1500 }, rows[] = { 2, 254, 258, 1300 }; const size_t shifts[] = { 0, 1, 7, 15 };
    for (int collide = 0; collide < 2 && !bad; collide++) {
        if (rfq_set_option(ctx, "RFQ_DEDUP", collide ? "collide" : nullptr)) return fail("RFQ_DEDUP", rfq_last_error(ctx));
        uint32_t k = 0;
        for (uint32_t L : lens) for (int pairs = 0; pairs < 2; pairs++) for (int mode = 0; mode < 2 && !bad; mode++, k++) {
            const uint32_t n = L > 1024 ? 40 : rows[k % 4], key_len = (k % 3 == 2) ? 1 + rnd() % (L + 3) : 0;
            const Rows r = make_rows(n, L, pairs ? 2 : 1, k % 2 == 1);
            char what[160]; snprintf(what, sizeof what, "collide %d row_len %u pairs %d mode %d rows %u key_len %u shift %zu", collide, L, pairs, mode, n, key_len, shifts[k % 4]);
            bad |= run(ctx, what, r, args(pairs, mode, key_len, (k % 3) ? 8 : 1024), 15, shifts[k % 4], mode == RFQ_DEDUP_BEST_QUAL || k % 4 == 0); calls++;
        }
        const Rows r = make_rows(300, 150, 1, false);
        for (int outs : { 1, 2, 4, 8, 0 }) { bad |= run(ctx, "one output alone", r, args(0, RFQ_DEDUP_BEST_QUAL, 0, 8), outs, 3); calls++; }
    }
    rfq_set_option(ctx, "RFQ_DEDUP", nullptr);
    for (uint32_t n : { 0u, 1u, 2u }) { const Rows z = make_rows(n, 16, 1, false); bad |= run(ctx, "0, 1, 2 rows", z, args(0, RFQ_DEDUP_FIRST, 0, 3), 15, 0); calls++; }
    { const Rows z = make_rows(0, 16, 2, false); bad |= run(ctx, "no pairs", z, args(1, RFQ_DEDUP_BEST_QUAL, 0, 3), 15, 0); calls++; }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 32, 1, true);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);                   // (a word more: the misaligned d_lens stays inside it)
        Dev db(ctx, r.B.data(), r.B.size()), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, lp.data(), 160 + 4), dc(ctx, r.cand.data(), 40), out(ctx, nullptr, 16384);
        const rfq_rows_in in = rows_in(40, 32, 0, db, &dq, dl);
        rfq_dedup_rows_args a; rfq_rows_in x;
        a = args(2, 0, 0, 0); bad |= refused(ctx, "pairs 2", in, a, "pairs"); refusals++;
        a = args(1, 0, 0, 0); x = in; x.n_rows = 39; bad |= refused(ctx, "an odd n_rows with pairs", x, a, "in pairs"); refusals++;
        a = args(0, 2, 0, 0); bad |= refused(ctx, "unknown mode", in, a, "mode"); refusals++;
        a = args(0, 1, 0, 0); x = in; x.d_quals = nullptr; bad |= refused(ctx, "BEST_QUAL without quals", x, a, "d_quals"); refusals++;
        a = args(0, 0, 0, 0); x = in; x.row_len = 0; bad |= refused(ctx, "row_len 0", x, a, "row_len"); refusals++;
        x = in; x.row_len = (1u << 22) + 1; bad |= refused(ctx, "row_len above 2^22", x, a, "2^22"); refusals++;
        x = in; x.d_bases = nullptr; bad |= refused(ctx, "null d_bases", x, a, "null"); refusals++;
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= refused(ctx, "misaligned d_lens", x, a, "aligned"); refusals++;
        a = args(0, 0, 0, 0); a.d_dup_of = (int32_t*)(out.p + 1); bad |= refused(ctx, "misaligned d_dup_of", in, a, "aligned"); refusals++;
        a = args(0, 0, 0, 0); a.d_count = (uint32_t*)(out.p + 2); bad |= refused(ctx, "misaligned d_count", in, a, "aligned"); refusals++;
        a = args(0, 0, 0, 8); a.d_hist = (uint64_t*)(out.p + 4); bad |= refused(ctx, "misaligned d_hist", in, a, "8-byte"); refusals++;
        a = args(0, 0, 0, 1025); a.d_hist = (uint64_t*)out.p; bad |= refused(ctx, "hist_len 1025", in, a, "hist_len"); refusals++;
        a = args(0, 0, 0, 0); a.d_hist = (uint64_t*)out.p; bad |= refused(ctx, "hist_len 0 with a histogram", in, a, "hist_len"); refusals++;
        a = args(0, 0, 0, 0); a.d_keep = db.p + 40 * 32 - 1; bad |= refused(ctx, "keep on bases", in, a, "overlaps"); refusals++;
        a = args(0, 0, 0, 0); a.d_in = dc.p; a.d_keep = dc.p; bad |= refused(ctx, "keep on d_in", in, a, "overlaps"); refusals++;
        a = args(0, 0, 0, 0); a.d_dup_of = (int32_t*)dl.p; bad |= refused(ctx, "dup_of on lens", in, a, "overlaps"); refusals++;
        a = args(0, 1, 0, 0); a.d_count = (uint32_t*)(dq.p + 16); bad |= refused(ctx, "count on quals", in, a, "overlaps"); refusals++;
        a = args(0, 0, 0, 8); a.d_hist = (uint64_t*)(db.p - 56); bad |= refused(ctx, "hist on bases", in, a, "overlaps"); refusals++;
        a = args(0, 0, 0, 0); x = in; x.n_rows = 0x7FFFFFFFull; x.row_len = 1; bad |= refused(ctx, "2^31 - 1 units", x, a, "too many"); refusals++;
        for (int collide = 0; collide < 2; collide++) for (int pairs = 0; pairs < 2; pairs++) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 20u, 21u, 39u }) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 160); x = in; x.d_lens = (const int32_t*)d2.p;
            a = args(pairs, RFQ_DEDUP_BEST_QUAL, 0, 8); a.d_in = (row & 1) ? dc.p : nullptr; a.d_keep = out.p; a.d_dup_of = (int32_t*)(out.p + 64); a.d_count = (uint32_t*)(out.p + 1024); a.d_hist = (uint64_t*)(out.p + 4096);
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_DEDUP", collide ? "collide" : nullptr);
            rfq_dedup_rows_result g;
            if (rfq_dedup_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_DEDUP", nullptr);
            bad |= good(ctx); refusals++;
        }
        if (rfq_set_option(ctx, "RFQ_DEDUP", "general") != RFQ_E_ARG) bad |= fail("RFQ_DEDUP=general", "not refused");
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("dedup_asan: %d good calls (12 row strides x rows / pairs x 2 modes x 2 option values at shifts 0 / 1 / 7 / 15, outputs alone, 0 / 1 / 2 rows), %d refusals (19 on the host, 32 on the device) each followed by a good call: all as the host reference says, no sanitizer report\n", calls, refusals);
    return 0;
}
