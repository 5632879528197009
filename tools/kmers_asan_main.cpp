// kmers_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_kmers_init, rfq_kmers_rows and rfq_kmers_read on the SIMT-interpreter build (CPU only, no
// Python): tools/kmers_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   kmers_asan_main         the good shapes of tests/_kmers.py - k of 4 .. 31, the row strides 15 .. 2080, both base modes, a mask, buffer shifts 0 / 1 / 7 / 15,
//   the default path, RFQ_KMERS=general and =direct and a table formatted under RFQ_KMERS=collide, calls that add up, hot values, the read with its bounds, its
//   spectrum, its list and its index handed to rfq_screen_rows - with rows and tables in allocations that end where their data ends and outputs of exactly the
//   entries a call may write, compared with a host reference (a std::map of canonical values, a loop over the positions) written from include/rfq_hip.h; then a
//   table that is full, and every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <map>
#include <string>
#include <vector>

static uint32_t cls_of(int codes, uint8_t c) {
    if (codes) return c < 4 ? c : 4;
    switch (c & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}
static bool canon(const uint8_t* s, int codes, uint32_t k, uint64_t* v) {
    uint64_t f = 0, rc = 0;
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t c = cls_of(codes, s[i]), d = cls_of(codes, s[k - 1 - i]);
        if (c > 3) return false;
        f = f * 4 + c; rc = rc * 4 + (3 - d);
    }
    *v = std::min(f, rc);
    return true;
}
static std::string random_seq(uint32_t n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() % 4]; return s; }
static uint64_t pow2(uint64_t want) { uint64_t s = 1024; while (s < want) s *= 2; return s; }
typedef std::map<uint64_t, uint64_t> Model;

struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, cand; std::vector<int32_t> lens; };
// n rows of stride L: random reads of 0 .. L bases, every third with a piece of `hot` or a poly-A tail, an "other" byte here and there, noise behind the reads
static Rows make_rows(uint32_t n, uint32_t L, int codes, bool mask, const std::string& hot) {
    Rows o; o.n = n; o.L = L; o.codes = codes; o.B.resize((size_t)n * L); o.lens.resize(n); if (mask) o.cand.resize(n);
    for (uint32_t g = 0; g < n; g++) {
        const uint32_t l = g % 4 == 0 ? L : rnd() % (L + 1); o.lens[g] = (int32_t)l;
        std::string s = random_seq(L);
        if (g % 3 == 0) for (uint32_t at = rnd() % 40; at < l; at += 64 + rnd() % 200) {
            const uint32_t m = std::min<uint32_t>({ 20 + rnd() % 60, l - at, (uint32_t)hot.size() }), from = rnd() % (hot.size() - m + 1);
            s.replace(at, m, hot.substr(from, m));
        }
        if (g % 6 == 1 && l > 40) for (uint32_t j = l - 40; j < l; j++) s[j] = 'A';
        if (g % 5 == 1 && l) s[rnd() % l] = 'N';
        if (g % 7 == 2) for (auto& c : s) c = (char)(c | 0x20);
        for (uint32_t j = 0; j < L; j++) {
            uint8_t b = (uint8_t)s[j];
            if (codes) b = (uint8_t)(cls_of(0, b) < 4 ? cls_of(0, b) : 4 + rnd() % 250);
            o.B[(size_t)g * L + j] = j < l ? b : (uint8_t)rnd();
        }
        if (mask) o.cand[g] = rnd() % 5 ? (uint8_t)(1 + rnd() % 255) : 0;
    }
    return o;
}
// a table in an allocation of exactly table_bytes, beside the host's model of everything counted into it
struct Table { Dev* d = nullptr; size_t bytes = 0; uint32_t k = 0; uint64_t S = 0; Model m; uint64_t total = 0; ~Table() { delete d; } };
static int init(rfq_ctx* ctx, const char* what, uint32_t k, uint64_t slots, Table* t) {
    rfq_kmers_init_args a; memset(&a, 0, sizeof a); a.k = k; a.slots = slots; a.size_only = 1;
    rfq_kmers_init_result q, g;
    if (rfq_kmers_init(ctx, &a, &q)) return fail(what, rfq_last_error(ctx));
    if (q.slots != pow2(slots) || q.table_bytes != 64 + 16 * q.slots) return fail(what, "the size query differs from the host's");
    if (!t->d || t->bytes != q.table_bytes) { delete t->d; t->d = new Dev(ctx, nullptr, q.table_bytes); }
    t->bytes = q.table_bytes; t->k = k; t->S = q.slots; t->m.clear(); t->total = 0;
    a.size_only = 0; a.d_table = t->d->p; a.table_cap = t->bytes;
    if (rfq_kmers_init(ctx, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (g.slots != q.slots || g.table_bytes != q.table_bytes) return fail(what, "the call reports otherwise than the size query");
    return 0;
}
static int count(rfq_ctx* ctx, const char* what, const Rows& r, Table* t, size_t shift, bool want_kmers) {
    const uint32_t n = r.n, k = t->k;
    std::vector<uint32_t> ek(n, 0); rfq_kmers_rows_result e; memset(&e, 0, sizeof e); e.n_rows = n;
    for (uint32_t g = 0; g < n; g++) {
        if (!r.cand.empty() && !r.cand[g]) continue;
        const uint32_t l = (uint32_t)r.lens[g];
        for (uint32_t p = 0; p + k <= l; p++) { uint64_t v; if (canon(&r.B[(size_t)g * r.L + p], r.codes, k, &v)) { ek[g]++; if (!t->m[v]++) e.n_new++; } }
        e.n_counted++; e.bases_in += l; e.added += ek[g];
    }
    t->total += e.added; e.n_kmers = t->m.size(); e.total = t->total;
    Dev db(ctx, r.B.data(), r.B.size(), shift), dl(ctx, r.lens.data(), n * 4ull), dc(ctx, r.cand.data(), r.cand.size()), ok(ctx, nullptr, n * 4ull);
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, nullptr, dl);
    rfq_kmers_rows_args a; memset(&a, 0, sizeof a); a.d_table = t->d->p; a.table_bytes = t->bytes; a.d_in = r.cand.empty() ? nullptr : dc.p; a.d_kmers = want_kmers ? (uint32_t*)ok.p : nullptr;
    rfq_kmers_rows_result g;
    if (rfq_kmers_rows(ctx, &in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e, sizeof g)) return fail(what, "the result differs from the host's");
    std::vector<uint32_t> hk(n + 1);
    if (want_kmers && n) { rfq_copy_d2h(ctx, hk.data(), ok.p, n * 4ull); if (memcmp(hk.data(), ek.data(), n * 4ull)) return fail(what, "kmers differ"); }
    return 0;
}
// the read in buffers of exactly the entries it may write, against the model; with_index: the index goes through rfq_screen_rows on `probe`
static int read(rfq_ctx* ctx, const char* what, const Table& t, uint64_t lo, uint64_t hi, uint32_t hist_len, const Rows* probe) {
    std::vector<std::pair<uint64_t, uint64_t>> sel; std::vector<uint64_t> eh(hist_len, 0);
    rfq_kmers_read_result e; memset(&e, 0, sizeof e); e.k = t.k; e.slots = t.S; e.n_kmers = t.m.size(); e.total = t.total;
    for (const auto& kv : t.m) {
        if (hist_len) eh[std::min<uint64_t>(kv.second, hist_len) - 1]++;
        e.max_count = std::max(e.max_count, kv.second);
        if (kv.second >= std::max<uint64_t>(lo, 1) && (hi == 0 || kv.second <= hi)) { sel.push_back(kv); e.n_selected++; e.selected_total += kv.second; }
    }
    e.index_slots = pow2(2 * e.n_selected); e.index_bytes = 64 + 8 * e.index_slots;
    rfq_kmers_read_args a; memset(&a, 0, sizeof a); a.d_table = t.d->p; a.table_bytes = t.bytes; a.min_count = lo; a.max_count = hi; a.size_only = 1;
    rfq_kmers_read_result q, g;
    if (rfq_kmers_read(ctx, &a, &q)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&q, &e, sizeof q)) return fail(what, "the size query differs from the host's");
    const size_t ns = sel.size();
    Dev dv(ctx, nullptr, ns * 8), dc(ctx, nullptr, ns * 8), dh(ctx, nullptr, hist_len * 8ull), di(ctx, nullptr, e.index_bytes);
    a.size_only = 0; a.hist_len = hist_len; a.d_hist = hist_len ? (uint64_t*)dh.p : nullptr; a.d_values = (uint64_t*)dv.p; a.d_counts = (uint64_t*)dc.p; a.list_cap = ns;
    if (probe) { a.d_index = di.p; a.index_cap = e.index_bytes; }
    if (rfq_kmers_read(ctx, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e, sizeof g)) return fail(what, "the read's result differs from the host's");
    std::vector<uint64_t> hv(ns + 1), hc(ns + 1), hh(hist_len + 1);
    if (ns) { rfq_copy_d2h(ctx, hv.data(), dv.p, ns * 8); rfq_copy_d2h(ctx, hc.data(), dc.p, ns * 8); }
    if (hist_len) { rfq_copy_d2h(ctx, hh.data(), dh.p, hist_len * 8ull); if (memcmp(hh.data(), eh.data(), hist_len * 8ull)) return fail(what, "the spectrum differs"); }
    std::vector<std::pair<uint64_t, uint64_t>> got(ns);
    for (size_t i = 0; i < ns; i++) got[i] = { hv[i], hc[i] };
    std::sort(got.begin(), got.end());
    if (got != sel) return fail(what, "the selected (value, count) pairs differ");
    if (probe) {
        const Rows& r = *probe; const uint32_t n = r.n;
        std::vector<uint32_t> eh2(n, 0);
        for (uint32_t gI = 0; gI < n; gI++) for (uint32_t p = 0; p + t.k <= (uint32_t)r.lens[gI]; p++) {
            uint64_t v; if (canon(&r.B[(size_t)gI * r.L + p], r.codes, t.k, &v)) { auto it = t.m.find(v); if (it != t.m.end() && it->second >= std::max<uint64_t>(lo, 1) && (hi == 0 || it->second <= hi)) eh2[gI]++; }
        }
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, r.lens.data(), n * 4ull), oh(ctx, nullptr, n * 4ull);
        const rfq_rows_in in = rows_in(n, r.L, r.codes, db, nullptr, dl);
        rfq_screen_rows_args s; memset(&s, 0, sizeof s); s.min_hits = 1; s.d_index = di.p; s.index_bytes = e.index_bytes; s.d_hits = (uint32_t*)oh.p;
        rfq_screen_rows_result sr;
        if (rfq_screen_rows(ctx, &in, &s, &sr)) return fail(what, rfq_last_error(ctx));
        std::vector<uint32_t> hh2(n + 1);
        if (n) { rfq_copy_d2h(ctx, hh2.data(), oh.p, n * 4ull); if (memcmp(hh2.data(), eh2.data(), n * 4ull)) return fail(what, "the hits against the read's index differ"); }
    }
    return 0;
}

static std::string hot;
static int good(rfq_ctx* ctx) {
    Table t;
    if (init(ctx, "a good table after a refusal", 16, 4096, &t)) return 1;
    const Rows r = make_rows(40, 48, 0, true, hot);
    return count(ctx, "a good count after a refusal", r, &t, 1, true) | read(ctx, "a good read after a refusal", t, 1, 0, 4, &r);
}
static int rows_refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_kmers_rows_args& a, int code, const char* needle) {
    rfq_kmers_rows_result g;
    if (rfq_kmers_rows(ctx, &in, &a, &g) != code) return fail(what, "not refused with the expected code");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}
static int read_refused(rfq_ctx* ctx, const char* what, const rfq_kmers_read_args& a, int code, const char* needle) {
    rfq_kmers_read_result g;
    if (rfq_kmers_read(ctx, &a, &g) != code) return fail(what, "not refused with the expected code");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}
static int init_refused(rfq_ctx* ctx, const char* what, const rfq_kmers_init_args& a, int code, const char* needle) {
    rfq_kmers_init_result g;
    if (rfq_kmers_init(ctx, &a, &g) != code) return fail(what, "not refused with the expected code");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, reads = 0, refusals = 0;
    hot = random_seq(300);
    const uint32_t ks[] = { 4, 5, 15, 16, 17, 25, 31 }, lens[] = { 15, 16, 17, 48, 150, 255, 256, 257, 300, 1023, 1024, 1025, 2080 }, rows[] = { 2, 62, 66, 130 }; const size_t shifts[] = { 0, 1, 7, 15 };
    const char* const ov[] = { nullptr, "general", "direct", "collide" };
    uint32_t j = 0;
    for (uint32_t k : ks) for (int form = 0; form < 4 && !bad; form++) {
        // one table per k and formulation: the strides' calls add up in it (every stride with k = 17 under the default, a third of them elsewhere)
        Table t; char what[200];
        rfq_set_option(ctx, "RFQ_KMERS", form == 3 ? "collide" : nullptr);
        bad |= init(ctx, "init", k, form == 3 ? 65536 : 1 << 20, &t);
        rfq_set_option(ctx, "RFQ_KMERS", nullptr);
        for (uint32_t L : lens) {
            j++;
            if (j % 3 != 0 && !(k == 17 && form == 0)) continue;
            if (form == 3 && L > 48) continue;                               // (under collide ONE chain holds everything: the short strides do)
            const int codes = (j / 3) % 2; const uint32_t n = L > 1024 ? 8 : rows[j % 4];
            const Rows r = make_rows(n, L, codes, j % 4 == 1, hot);
            snprintf(what, sizeof what, "k %u under %s, row_len %u codes %d rows %u shift %zu", k, ov[form] ? ov[form] : "default", L, codes, n, shifts[j % 4]);
            rfq_set_option(ctx, "RFQ_KMERS", form == 3 ? nullptr : ov[form]);
            bad |= count(ctx, what, r, &t, shifts[j % 4], j % 5 != 0); calls++;
            rfq_set_option(ctx, "RFQ_KMERS", nullptr);
            if (bad) break;
        }
        if (bad) break;
        const Rows probe = make_rows(30, 100, 0, false, hot);
        snprintf(what, sizeof what, "the read of the table of k %u under %s", k, ov[form] ? ov[form] : "default");
        bad |= read(ctx, what, t, 1, 0, 16, nullptr) | read(ctx, what, t, 2, 0, 1, &probe) | read(ctx, what, t, 2, 5, 5000, &probe) | read(ctx, what, t, 1 << 30, 0, 0, &probe); reads += 4;
    }
    if (!bad) {   // hot values: one value from every lane; an empty table; 0 rows
        Table t; Rows r; r.n = 300; r.L = 160; r.B.assign((size_t)300 * 160, 'A'); r.lens.assign(300, 150);
        bad |= init(ctx, "hot", 25, 1024, &t) | count(ctx, "300 rows of poly-A", r, &t, 0, true) | read(ctx, "the read of one hot value", t, 1, 0, 4, &r); calls++; reads++;
        bad |= init(ctx, "empty", 25, 0, &t) | read(ctx, "the read of an empty table", t, 1, 0, 3, &r); reads++;
        Rows z; z.n = 0; z.L = 16;
        bad |= count(ctx, "no rows", z, &t, 0, true); calls++;
    }
    if (!bad) {   // a table that is full: refused, marked, refused again, formatted again
        Table t; bad |= init(ctx, "full", 25, 1024, &t);
        Rows r; r.n = 30; r.L = 128; r.lens.assign(30, 128);               // 30 * 104 k-mers of random sequence: 3120 distinct values
        { const std::string s = random_seq(30 * 128); r.B.assign(s.begin(), s.end()); }
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, r.lens.data(), 120);
        const rfq_rows_in in = rows_in(30, 128, 0, db, nullptr, dl);
        rfq_kmers_rows_args a; memset(&a, 0, sizeof a); a.d_table = t.d->p; a.table_bytes = t.bytes;
        rfq_kmers_rows_result g; rfq_kmers_read_args ra; memset(&ra, 0, sizeof ra); ra.d_table = t.d->p; ra.table_bytes = t.bytes; ra.size_only = 1; rfq_kmers_read_result rg;
        for (const char* o : { (const char*)nullptr, "general", "direct" }) {
            rfq_set_option(ctx, "RFQ_KMERS", o);
            if (rfq_kmers_rows(ctx, &in, &a, &g) != RFQ_E_NOSPACE || !g.lost || !strstr(rfq_last_error(ctx), "k-mers lost")) bad |= fail("a full table", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_KMERS", nullptr);
            if (rfq_kmers_rows(ctx, &in, &a, &g) != RFQ_E_DATA || !strstr(rfq_last_error(ctx), "INCOMPLETE")) bad |= fail("rows into an incomplete table", rfq_last_error(ctx));
            if (rfq_kmers_read(ctx, &ra, &rg) != RFQ_E_DATA || !strstr(rfq_last_error(ctx), "INCOMPLETE")) bad |= fail("the read of an incomplete table", rfq_last_error(ctx));
            bad |= init(ctx, "formatted again", 25, 1024, &t) | good(ctx); refusals += 3;
        }
        const Rows few = make_rows(4, 128, 0, false, hot);
        bad |= count(ctx, "a count after the table was formatted again", few, &t, 0, true) | read(ctx, "its read", t, 1, 0, 4, nullptr);
    }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 32, 0, true, hot);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, lp.data(), 160 + 4), dc(ctx, r.cand.data(), 40), out(ctx, nullptr, 16384);
        const rfq_rows_in in = rows_in(40, 32, 0, db, nullptr, dl);
        Table t; bad |= init(ctx, "the refusals' table", 16, 2048, &t) | count(ctx, "the refusals' table", r, &t, 0, true);
        rfq_kmers_rows_args a0; memset(&a0, 0, sizeof a0); a0.d_table = t.d->p; a0.table_bytes = t.bytes;
        rfq_kmers_rows_args a; rfq_rows_in x;
        a = a0; x = in; x.base_mode = 7; bad |= rows_refused(ctx, "a bad base_mode", x, a, RFQ_E_ARG, "base_mode"); refusals++;
        x = in; x.row_len = 0; bad |= rows_refused(ctx, "row_len 0", x, a, RFQ_E_ARG, "row_len"); refusals++;
        x = in; x.d_bases = nullptr; bad |= rows_refused(ctx, "null d_bases", x, a, RFQ_E_ARG, "null"); refusals++;
        x = in; x.d_lens = nullptr; bad |= rows_refused(ctx, "null d_lens", x, a, RFQ_E_ARG, "null"); refusals++;
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= rows_refused(ctx, "misaligned d_lens", x, a, RFQ_E_ARG, "aligned"); refusals++;
        a = a0; a.d_table = nullptr; bad |= rows_refused(ctx, "null table", in, a, RFQ_E_ARG, "d_table"); refusals++;
        a = a0; a.d_table = t.d->p + 8; a.table_bytes -= 8; bad |= rows_refused(ctx, "misaligned table", in, a, RFQ_E_ARG, "d_table"); refusals++;
        a = a0; a.table_bytes = 63; bad |= rows_refused(ctx, "table_bytes 63", in, a, RFQ_E_ARG, "d_table"); refusals++;
        a = a0; a.d_kmers = (uint32_t*)(out.p + 2); bad |= rows_refused(ctx, "misaligned d_kmers", in, a, RFQ_E_ARG, "aligned"); refusals++;
        a = a0; a.d_kmers = (uint32_t*)(db.p + 40 * 32 - 4); bad |= rows_refused(ctx, "kmers on bases", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = a0; a.d_in = dc.p; a.d_kmers = (uint32_t*)dc.p; bad |= rows_refused(ctx, "kmers on d_in", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = a0; a.d_kmers = (uint32_t*)dl.p; bad |= rows_refused(ctx, "kmers on lens", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = a0; a.d_kmers = (uint32_t*)(t.d->p + t.bytes - 4); bad |= rows_refused(ctx, "kmers on the table", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = a0; a.d_in = t.d->p + 4096; bad |= rows_refused(ctx, "the table on d_in", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = a0; x = in; x.n_rows = 1ull << 31; x.row_len = 1; bad |= rows_refused(ctx, "2^31 rows", x, a, RFQ_E_ARG, "too many"); refusals++;
        rfq_kmers_read_args r0; memset(&r0, 0, sizeof r0); r0.d_table = t.d->p; r0.table_bytes = t.bytes;
        rfq_kmers_read_args ra;
        ra = r0; ra.d_table = nullptr; bad |= read_refused(ctx, "read: null table", ra, RFQ_E_ARG, "d_table"); refusals++;
        ra = r0; ra.table_bytes = 63; bad |= read_refused(ctx, "read: table_bytes 63", ra, RFQ_E_ARG, "d_table"); refusals++;
        ra = r0; ra.hist_len = 65537; bad |= read_refused(ctx, "read: hist_len 65537", ra, RFQ_E_ARG, "hist_len"); refusals++;
        ra = r0; ra.d_hist = (uint64_t*)out.p; bad |= read_refused(ctx, "read: hist_len 0 with d_hist", ra, RFQ_E_ARG, "hist_len"); refusals++;
        ra = r0; ra.hist_len = 4; ra.d_hist = (uint64_t*)(out.p + 4); bad |= read_refused(ctx, "read: misaligned d_hist", ra, RFQ_E_ARG, "8-byte"); refusals++;
        ra = r0; ra.d_values = (uint64_t*)(out.p + 1); ra.list_cap = 4; bad |= read_refused(ctx, "read: misaligned d_values", ra, RFQ_E_ARG, "8-byte"); refusals++;
        ra = r0; ra.d_index = out.p + 8; ra.index_cap = 8256; bad |= read_refused(ctx, "read: misaligned d_index", ra, RFQ_E_ARG, "16-byte"); refusals++;
        ra = r0; ra.hist_len = 4; ra.d_hist = (uint64_t*)(t.d->p + t.bytes - 8); bad |= read_refused(ctx, "read: hist on the table", ra, RFQ_E_ARG, "overlaps"); refusals++;
        ra = r0; ra.d_values = (uint64_t*)out.p; ra.d_counts = (uint64_t*)(out.p + 8); ra.list_cap = 4; bad |= read_refused(ctx, "read: values on counts", ra, RFQ_E_ARG, "overlaps"); refusals++;
        ra = r0; ra.d_values = (uint64_t*)out.p; ra.d_counts = (uint64_t*)(out.p + 8192); ra.list_cap = t.m.size() - 1; bad |= read_refused(ctx, "read: a list one entry short", ra, RFQ_E_NOSPACE, "need"); refusals++;
        ra = r0; ra.d_index = out.p; ra.index_cap = 64 + 8 * pow2(2 * t.m.size()) - 1; bad |= read_refused(ctx, "read: an index one byte short", ra, RFQ_E_NOSPACE, "need"); refusals++;
        {   // headers rfq_kmers_init does not write, a zeroed one, a screen index; slots of garbage
            std::vector<uint8_t> img(t.bytes); rfq_copy_d2h(ctx, img.data(), t.d->p, t.bytes);
            struct Edit { size_t word; uint32_t v; const char* needle; } const edits[] = { { 0, 0x12345678u, "header" }, { 2, 2u, "header" }, { 3, 0u, "k" }, { 3, 32u, "k" }, { 4, 1000u, "slot count" },
                                                                                           { 4, 0u, "slot count" }, { 4, 4096u, "slot count" }, { 5, 1u, "slot count" }, { 10, 2u, "INCOMPLETE" } };
            for (const Edit& e : edits) {
                std::vector<uint8_t> m = img; memcpy(&m[4 * e.word], &e.v, 4);
                Dev dm(ctx, m.data(), m.size());
                a = a0; a.d_table = dm.p; bad |= rows_refused(ctx, "a header that is not the init's", in, a, RFQ_E_DATA, e.needle); refusals++;
                ra = r0; ra.d_table = dm.p; bad |= read_refused(ctx, "a header that is not the init's", ra, RFQ_E_DATA, e.needle); refusals++;
            }
            { std::vector<uint8_t> m = img; memset(m.data(), 0, 64); Dev dm(ctx, m.data(), m.size());
              a = a0; a.d_table = dm.p; bad |= rows_refused(ctx, "a zeroed header", in, a, RFQ_E_DATA, "header"); refusals++; }
            {   // a screen index as a table
                const std::string ref = random_seq(100); const uint64_t off[2] = { 0, 100 };
                Dev rb(ctx, ref.data(), 100), ro(ctx, off, 16), ix(ctx, nullptr, 64 + 8 * 1024);
                rfq_screen_build_args b; memset(&b, 0, sizeof b); b.k = 16; b.d_refs = rb.p; b.refs_len = 100; b.d_ref_off = (const uint64_t*)ro.p; b.n_refs = 1; b.d_index = ix.p; b.index_cap = 64 + 8 * 1024;
                rfq_screen_build_result br;
                if (rfq_screen_build(ctx, &b, &br)) bad |= fail("a screen index", rfq_last_error(ctx));
                a = a0; a.d_table = ix.p; a.table_bytes = 64 + 8 * 1024; bad |= rows_refused(ctx, "a screen index as a table", in, a, RFQ_E_DATA, "header"); refusals++;
                rfq_screen_rows_args s; memset(&s, 0, sizeof s); s.min_hits = 1; s.d_index = t.d->p; s.index_bytes = t.bytes; rfq_screen_rows_result sr;
                if (rfq_screen_rows(ctx, &in, &s, &sr) != RFQ_E_DATA) bad |= fail("a table as a screen index", "not refused");
                refusals++;
            }
            std::vector<uint8_t> m = img;
            for (uint64_t i = 0; i < t.S; i++) { const uint64_t v = (1ull << 63) | (1ull << 40) | i, c = ((uint64_t)rnd() << 20) | 1; memcpy(&m[64 + 8 * i], &v, 8); memcpy(&m[64 + 8 * (t.S + i)], &c, 8); }
            for (const char* o : { (const char*)nullptr, "general", "direct" }) {
                Dev dm(ctx, m.data(), m.size());
                rfq_set_option(ctx, "RFQ_KMERS", o);
                a = a0; a.d_table = dm.p; rfq_kmers_rows_result g;
                if (rfq_kmers_rows(ctx, &in, &a, &g) != RFQ_E_NOSPACE || g.lost == 0 || g.added != 0) bad |= fail("a table of garbage", rfq_last_error(ctx));      // (every walk ends after min(S, W) steps: the call comes back)
                rfq_set_option(ctx, "RFQ_KMERS", nullptr);
                std::vector<uint8_t> back(m.size()); rfq_copy_d2h(ctx, back.data(), dm.p, m.size());
                if (memcmp(&back[64], &m[64], m.size() - 64)) bad |= fail("a table of garbage", "the slots or the counts were written");
                ra = r0; ra.d_table = dm.p; bad |= read_refused(ctx, "the read of a table of garbage", ra, RFQ_E_DATA, nullptr); refusals += 2;
            }
        }
        for (const char* o : { (const char*)nullptr, "general", "direct" }) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 20u, 39u }) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 160); x = in; x.d_lens = (const int32_t*)d2.p;
            a = a0; a.d_in = (row & 1) ? dc.p : nullptr; a.d_kmers = (uint32_t*)out.p;
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_KMERS", o);
            rfq_kmers_rows_result g;
            if (rfq_kmers_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_KMERS", nullptr);
            bad |= good(ctx); refusals++;
        }
        // rfq_kmers_init's refusals
        Dev tb(ctx, nullptr, 64 + 16 * 1024);
        rfq_kmers_init_args i0; memset(&i0, 0, sizeof i0); i0.k = 16; i0.slots = 10; i0.d_table = tb.p; i0.table_cap = 64 + 16 * 1024;
        rfq_kmers_init_args i;
        i = i0; i.k = 3; bad |= init_refused(ctx, "k 3", i, RFQ_E_ARG, "k must be"); refusals++;
        i = i0; i.k = 32; i.size_only = 1; bad |= init_refused(ctx, "k 32", i, RFQ_E_ARG, "k must be"); refusals++;
        i = i0; i.slots = (1ull << 36) + 1; i.size_only = 1; bad |= init_refused(ctx, "slots 2^36 + 1", i, RFQ_E_ARG, "2^36"); refusals++;
        i = i0; i.d_table = nullptr; bad |= init_refused(ctx, "null d_table", i, RFQ_E_ARG, "null d_table"); refusals++;
        i = i0; i.d_table = tb.p + 8; bad |= init_refused(ctx, "misaligned d_table", i, RFQ_E_ARG, "16-byte"); refusals++;
        i = i0; i.table_cap -= 1; bad |= init_refused(ctx, "a table buffer one byte short", i, RFQ_E_NOSPACE, "need 16448 bytes"); refusals++;
        rfq_set_option(ctx, "RFQ_KMERS", "collide");
        i = i0; i.slots = 65537; i.size_only = 1; { rfq_kmers_init_result g; if (rfq_kmers_init(ctx, &i, &g) != RFQ_E_ARG) bad |= fail("collide with 65537 slots", "not refused"); } refusals++;
        rfq_set_option(ctx, "RFQ_KMERS", nullptr);
        if (rfq_set_option(ctx, "RFQ_KMERS", "staged") != RFQ_E_ARG) bad |= fail("RFQ_KMERS=staged", "not refused");
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("kmers_asan: %d good counts (k 4 .. 31 x default / general / direct / a table formatted under collide, 13 row strides, both base modes, masks, shifts 0 / 1 / 7 / 15, calls that add up, "
           "a hot value, no rows) and %d reads (bounds, spectra of 1 .. 5000 bins, lists, the index through rfq_screen_rows, an empty table), %d refusals (a full table, host, header, garbage, "
           "device and init) each followed by a good table, count and read: all as the host reference says, no sanitizer report\n", calls, reads, refusals);
    return 0;
}
