// profile_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_profile_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/profile_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   profile_asan_main       the good shapes of tests/_profile.py - row strides 1 .. 1040, rows and pairs, both base modes, with and without the keep / start / length
//   triple, cycles and bins below and above the rows' own, buffer shifts 0 / 1 / 7 / 15, the default path and RFQ_PROFILE=general, each table alone and none - with
//   rows in allocations that end where the rows end and tables of exactly the entries a call may write, compared with a host reference (a loop over rows and
//   positions) written from include/rfq_hip.h; then every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
// (The interpreter keeps LDS in host thread-local memory: a sanitizer sees no LDS overrun.  enc/rows_profile.h bounds every LDS index by construction.)
#include "asan_common.h"
#include <algorithm>
#include <vector>

struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, Q, keep; std::vector<int32_t> lens, start, len; };
static Rows make_rows(uint32_t n, uint32_t L, int codes, bool triple) {
    Rows r; r.n = n; r.L = L; r.codes = codes; r.B.resize((size_t)n * L); r.Q.resize((size_t)n * L); r.lens.resize(n);
    static const char alpha[] = "AACCGGTTNacgtnRYK."; static const uint8_t code[] = { 0, 0, 1, 1, 2, 2, 3, 3, 4, 5, 255 };
    for (auto& b : r.B) b = codes ? code[rnd() % 11] : (uint8_t)alpha[rnd() % 18];
    for (auto& q : r.Q) { const uint32_t x = rnd() % 50; q = x == 0 ? 255 : (x == 1 ? 0 : (uint8_t)(rnd() % 46)); }
    for (uint32_t i = 0; i < n; i++) r.lens[i] = i == 0 ? (int32_t)L : (i == 2 ? 0 : (int32_t)(rnd() % (L + 1)));
    if (triple) {
        r.keep.resize(n); r.start.resize(n); r.len.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t l = (uint32_t)r.lens[i];
            r.keep[i] = rnd() % 4 ? (uint8_t)(1 + rnd() % 255) : 0;
            r.start[i] = rnd() % 3 ? (int32_t)(rnd() % (l + 1)) : 0;
            r.len[i] = rnd() % 8 ? (int32_t)(rnd() % (l - (uint32_t)r.start[i] + 1)) : 0;
            if (rnd() % 4 == 0) { r.start[i] = 0; r.len[i] = (int32_t)l; }
        }
    }
    return r;
}
static uint32_t cls_of(int codes, uint8_t b) {
    if (codes) return b < 4 ? b : 4;
    switch (b & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}
struct Ref { std::vector<uint64_t> t[6]; rfq_profile_rows_result s; };
static size_t table_len(const rfq_profile_rows_args& a, int k) {
    const size_t M = a.pairs ? 2 : 1;
    switch (k) { case 0: case 1: return M * a.cycles * 5; case 2: return M * a.cycles * a.qbins; case 3: return M * a.len_bins; case 4: return M * a.qbins; default: return M * 101; }
}
static Ref reference(const Rows& r, const rfq_profile_rows_args& a, bool quals) {
    Ref o; memset(&o.s, 0, sizeof o.s); o.s.n_rows = r.n;
    for (int k = 0; k < 6; k++) o.t[k].assign(table_len(a, k), 0);
    for (uint32_t i = 0; i < r.n; i++) {
        if (!r.keep.empty() && !r.keep[i]) continue;
        const uint32_t m = a.pairs ? i & 1 : 0, s = r.start.empty() ? 0 : (uint32_t)r.start[i], w = r.len.empty() ? (uint32_t)r.lens[i] - s : (uint32_t)r.len[i];
        uint64_t qsum = 0, acgt = 0, gc = 0;
        for (uint32_t c = 0; c < w; c++) {
            const uint32_t cc = std::min(c, a.cycles - 1), k = cls_of(r.codes, r.B[(size_t)i * r.L + s + c]), q = quals ? r.Q[(size_t)i * r.L + s + c] : 0;
            o.t[0][((size_t)m * a.cycles + cc) * 5 + k]++; o.t[1][((size_t)m * a.cycles + cc) * 5 + k] += q;
            o.t[2][((size_t)m * a.cycles + cc) * a.qbins + std::min(q, a.qbins - 1)]++;
            qsum += q; acgt += k < 4; gc += k == 1 || k == 2; o.s.q20[m] += q >= 20; o.s.q30[m] += q >= 30;
        }
        o.s.counted[m]++; o.s.bases[m] += w; o.s.qsum[m] += qsum; o.s.gc[m] += gc; o.s.other[m] += w - acgt; o.s.max_len = std::max<uint64_t>(o.s.max_len, w);
        o.t[3][(size_t)m * a.len_bins + std::min(w, a.len_bins - 1)]++;
        if (w) o.t[4][(size_t)m * a.qbins + std::min<uint64_t>(qsum / w, a.qbins - 1)]++;
        if (acgt) o.t[5][(size_t)m * 101 + 100 * gc / acgt]++;
    }
    return o;
}
static rfq_profile_rows_args args(int pairs, uint32_t cycles, uint32_t qbins, uint32_t len_bins) {
    rfq_profile_rows_args a; memset(&a, 0, sizeof a); a.pairs = pairs; a.cycles = cycles; a.qbins = qbins; a.len_bins = len_bins; return a;
}
static uint64_t** slot(rfq_profile_rows_args& a, int k) {
    uint64_t** p[] = { &a.d_base_cnt, &a.d_base_qsum, &a.d_qual_hist, &a.d_len_hist, &a.d_meanq_hist, &a.d_gc_hist }; return p[k];
}
// tabs: bit k = table k is asked for (quality tables only with quals)
static int run(rfq_ctx* ctx, const char* what, const Rows& r, rfq_profile_rows_args a, int tabs, size_t shift, bool quals = true) {
    const uint32_t n = r.n; const Ref e = reference(r, a, quals);
    if (!quals) tabs &= ~(2 | 4 | 16);
    Dev db(ctx, r.B.data(), r.B.size(), shift), dq(ctx, r.Q.data(), r.Q.size(), shift), dl(ctx, r.lens.data(), n * 4ull);
    Dev dk(ctx, r.keep.data(), r.keep.size()), ds(ctx, r.start.data(), r.start.size() * 4), dn(ctx, r.len.data(), r.len.size() * 4);
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, quals ? &dq : nullptr, dl);
    a.d_keep = r.keep.empty() ? nullptr : dk.p; a.d_start = r.start.empty() ? nullptr : (const int32_t*)ds.p; a.d_len = r.len.empty() ? nullptr : (const int32_t*)dn.p;
    std::vector<Dev*> out;
    for (int k = 0; k < 6; k++) { out.push_back(new Dev(ctx, nullptr, table_len(a, k) * 8)); *slot(a, k) = (tabs >> k) & 1 ? (uint64_t*)out[k]->p : nullptr; }
    rfq_profile_rows_result g; int bad = 0;
    if (rfq_profile_rows(ctx, &in, &a, &g)) bad = fail(what, rfq_last_error(ctx));
    else if (memcmp(&g, &e.s, sizeof g)) bad = fail(what, "the summary differs from the host's");
    for (int k = 0; k < 6 && !bad; k++) if ((tabs >> k) & 1) {
        std::vector<uint64_t> h(table_len(a, k) + 1);
        rfq_copy_d2h(ctx, h.data(), out[k]->p, table_len(a, k) * 8);
        if (memcmp(h.data(), e.t[k].data(), table_len(a, k) * 8)) { char w[200]; snprintf(w, sizeof w, "table %d differs", k); bad = fail(what, w); }
    }
    for (Dev* d : out) delete d;
    return bad;
}
static int good(rfq_ctx* ctx) { const Rows r = make_rows(60, 33, 0, true); return run(ctx, "a good call after a refusal", r, args(1, 33, 8, 34), 63, 0); }
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_profile_rows_args& a, const char* needle) {
    rfq_profile_rows_result g;
    const int rc = rfq_profile_rows(ctx, &in, &a, &g);
    if (rc != RFQ_E_ARG) return fail(what, "not refused with RFQ_E_ARG");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, refusals = 0;
    const uint32_t lens[] = { 1, 15, 16, 17, 100, 150, 256, 272, 1024, 1040 }, rows[] = { 2, 62, 66, 210 }; const size_t shifts[] = { 0, 1, 7, 15 };
    for (int general = 0; general < 2 && !bad; general++) {
        if (rfq_set_option(ctx, "RFQ_PROFILE", general ? "general" : nullptr)) return fail("RFQ_PROFILE", rfq_last_error(ctx));
        uint32_t k = 0;
        for (uint32_t L : lens) for (int pairs = 0; pairs < 2; pairs++) for (int codes = 0; codes < 2 && !bad; codes++, k++) {
            const uint32_t n = L > 256 ? 10 : rows[k % 4], cycles = (k % 3 == 0) ? L : (k % 3 == 1 ? std::max(1u, L / 3) : L + 9), qbins = (k % 4 == 0) ? 256 : (k % 4 == 1 ? 42 : (k % 4 == 2 ? 1 : 64));
            const Rows r = make_rows(n, L, codes, k % 2 == 1);
            char what[200]; snprintf(what, sizeof what, "general %d row_len %u pairs %d codes %d rows %u cycles %u qbins %u shift %zu", general, L, pairs, codes, n, cycles, qbins, shifts[k % 4]);
            bad |= run(ctx, what, r, args(pairs, cycles, qbins, (k % 5 == 0) ? 1 : L + 1), 63, shifts[k % 4], k % 7 != 3); calls++;
        }
        const Rows r = make_rows(120, 150, 1, true);
        for (int tabs : { 1, 2, 4, 8, 16, 32, 0 }) { bad |= run(ctx, "one table alone", r, args(1, 150, 42, 151), tabs, 3); calls++; }
    }
    rfq_set_option(ctx, "RFQ_PROFILE", nullptr);
    for (uint32_t n : { 0u, 1u, 2u }) { const Rows z = make_rows(n, 16, 0, false); bad |= run(ctx, "0, 1, 2 rows", z, args(0, 16, 8, 17), 63, 0); calls++; }
    { const Rows z = make_rows(40, 300, 1, false); bad |= run(ctx, "tables beyond the LDS", z, args(1, 300, 256, 301), 63, 0); calls++; }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 32, 0, true);
        std::vector<int32_t> lp = r.lens, sp = r.start, np = r.len; lp.push_back(0); sp.push_back(0); np.push_back(0);      // (a word more: a misaligned array stays inside it)
        Dev db(ctx, r.B.data(), r.B.size()), dq(ctx, r.Q.data(), r.Q.size()), dl(ctx, lp.data(), 160 + 4), dk(ctx, r.keep.data(), 40), ds(ctx, sp.data(), 160 + 4), dn(ctx, np.data(), 160 + 4), out(ctx, nullptr, 65536);
        const rfq_rows_in in = rows_in(40, 32, 0, db, &dq, dl);
        rfq_profile_rows_args a; rfq_rows_in x;
        uint64_t* const T = (uint64_t*)out.p;
        a = args(2, 4, 4, 4); bad |= refused(ctx, "pairs 2", in, a, "pairs"); refusals++;
        a = args(1, 4, 4, 4); x = in; x.n_rows = 39; bad |= refused(ctx, "an odd n_rows with pairs", x, a, "in pairs"); refusals++;
        a = args(0, 4, 4, 4); x = in; x.base_mode = 7; bad |= refused(ctx, "a bad base_mode", x, a, "base_mode"); refusals++;
        x = in; x.row_len = 0; bad |= refused(ctx, "row_len 0", x, a, "row_len"); refusals++;
        x = in; x.d_lens = nullptr; bad |= refused(ctx, "null d_lens", x, a, "null d_lens"); refusals++;
        x = in; x.n_rows = 1ull << 31; x.row_len = 1; bad |= refused(ctx, "2^31 rows", x, a, "too many"); refusals++;
        for (uint32_t c : { 0u, 65537u }) { a = args(0, c, 4, 4); a.d_base_cnt = T; bad |= refused(ctx, "cycles out of range", in, a, "cycles"); refusals++; }
        for (uint32_t c : { 0u, 257u }) { a = args(0, 4, c, 4); a.d_meanq_hist = T; bad |= refused(ctx, "qbins out of range", in, a, "qbins"); refusals++; }
        for (uint32_t c : { 0u, (1u << 20) + 1u }) { a = args(0, 4, 4, c); a.d_len_hist = T; bad |= refused(ctx, "len_bins out of range", in, a, "len_bins"); refusals++; }
        for (int k : { 1, 2, 4 }) { a = args(0, 4, 4, 4); *slot(a, k) = T; x = in; x.d_quals = nullptr; bad |= refused(ctx, "a score table without quals", x, a, "d_quals"); refusals++; }
        for (int k : { 0, 1, 5 }) { a = args(0, 4, 4, 4); *slot(a, k) = T; x = in; x.d_bases = nullptr; bad |= refused(ctx, "a base table without bases", x, a, "d_bases"); refusals++; }
        a = args(0, 4, 4, 4); x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= refused(ctx, "misaligned d_lens", x, a, "4-byte"); refusals++;
        a = args(0, 4, 4, 4); a.d_start = (const int32_t*)(ds.p + 1); bad |= refused(ctx, "misaligned d_start", in, a, "4-byte"); refusals++;
        a = args(0, 4, 4, 4); a.d_len = (const int32_t*)(dn.p + 2); bad |= refused(ctx, "misaligned d_len", in, a, "4-byte"); refusals++;
        for (int k = 0; k < 6; k++) { a = args(0, 4, 4, 4); *slot(a, k) = (uint64_t*)(out.p + 4); bad |= refused(ctx, "a misaligned table", in, a, "8-byte"); refusals++; }
        a = args(0, 4, 4, 4); a.d_base_cnt = (uint64_t*)(db.p + 40 * 32 - 8); bad |= refused(ctx, "a table on bases", in, a, "overlaps the input rows->d_bases"); refusals++;
        a = args(0, 4, 4, 4); a.d_qual_hist = (uint64_t*)(dq.p + 16); bad |= refused(ctx, "a table on quals", in, a, "overlaps the input rows->d_quals"); refusals++;
        a = args(0, 4, 4, 4); a.d_len_hist = (uint64_t*)dl.p; bad |= refused(ctx, "a table on lens", in, a, "overlaps the input rows->d_lens"); refusals++;
        a = args(0, 4, 4, 4); a.d_keep = dk.p; a.d_gc_hist = (uint64_t*)dk.p; bad |= refused(ctx, "a table on keep", in, a, "overlaps the input d_keep"); refusals++;
        a = args(0, 4, 4, 4); a.d_start = (const int32_t*)ds.p; a.d_meanq_hist = (uint64_t*)(ds.p + 152); bad |= refused(ctx, "a table on start", in, a, "overlaps the input d_start"); refusals++;
        a = args(0, 4, 4, 4); a.d_len = (const int32_t*)dn.p; a.d_base_qsum = (uint64_t*)(dn.p + 8); bad |= refused(ctx, "a table on len", in, a, "overlaps the input d_len"); refusals++;
        a = args(0, 4, 4, 4); a.d_base_cnt = T; a.d_base_qsum = T + 19; bad |= refused(ctx, "a table on a table", in, a, "overlaps the output"); refusals++;
        // on the device: a bad length, a bad window - first, in the last wave, last; counted or not; both paths
        for (int general = 0; general < 2; general++) for (int kind = 0; kind < 5; kind++) for (uint32_t row : { 0u, 21u, 39u }) {
            std::vector<int32_t> l2 = r.lens, s2 = r.start, n2 = r.len;
            switch (kind) { case 0: l2[row] = -1; break; case 1: l2[row] = 33; break; case 2: s2[row] = -1; break; case 3: n2[row] = -1; break;
                            default: s2[row] = n2[row] = 0x7FFFFFFF; }
            Dev d2(ctx, l2.data(), 160), d3(ctx, s2.data(), 160), d4(ctx, n2.data(), 160);
            x = in; x.d_lens = (const int32_t*)d2.p;
            a = args(1, 32, 8, 33); a.d_keep = (row & 1) ? dk.p : nullptr; a.d_start = (const int32_t*)d3.p; a.d_len = (const int32_t*)d4.p;
            a.d_base_cnt = T; a.d_base_qsum = T + 512; a.d_qual_hist = T + 1024; a.d_len_hist = T + 2048; a.d_meanq_hist = T + 2304; a.d_gc_hist = T + 2560;
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_PROFILE", general ? "general" : nullptr);
            rfq_profile_rows_result g;
            if (rfq_profile_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle) || !strstr(rfq_last_error(ctx), kind < 2 ? "read length" : "window"))
                bad |= fail("a bad length or window", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_PROFILE", nullptr);
            bad |= good(ctx); refusals++;
        }
        if (rfq_set_option(ctx, "RFQ_PROFILE", "collide") != RFQ_E_ARG) bad |= fail("RFQ_PROFILE=collide", "not refused");
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("profile_asan: %d good calls (10 row strides x rows / pairs x 2 base modes x 2 option values at shifts 0 / 1 / 7 / 15, tables alone, 0 / 1 / 2 rows, tables beyond the LDS), %d refusals (34 on the host, 30 on the device) each followed by a good call: all as the host reference says, no sanitizer report\n", calls, refusals);
    return 0;
}
