// screen_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_screen_build and rfq_screen_rows on the SIMT-interpreter build (CPU only, no Python):
// tools/screen_asan.sh compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   screen_asan_main        the good shapes of tests/_screen.py - k of 4 .. 31, the row strides 15 .. 2080, rows and pairs, both modes and both base modes, a candidate
//   mask, thresholds, buffer shifts 0 / 1 / 7 / 15, an index that fits the LDS and one that does not, the default path, RFQ_SCREEN=general and an index built under
//   RFQ_SCREEN=collide, each output alone and none - with rows, references and indexes in allocations that end where their data ends and outputs of exactly the
//   entries a call may write, compared with a host reference (a std::set of canonical values, a loop over the positions) written from include/rfq_hip.h; then
//   every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <set>
#include <string>
#include <vector>

static uint32_t cls_of(int codes, uint8_t c) {
    if (codes) return c < 4 ? c : 4;
    switch (c & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}
// the canonical value of the k-mer at p, false when it is not valid
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
struct Refs { std::string blob; std::vector<uint64_t> off{ 0 }; void add(const std::string& s) { blob += s; off.push_back(blob.size()); } };
struct Set { std::set<uint64_t> s; uint64_t positions = 0; };
static Set set_of(const Refs& r, uint32_t k) {
    Set o;
    for (size_t i = 0; i + 1 < r.off.size(); i++)
        for (uint64_t p = r.off[i]; p + k <= r.off[i + 1]; p++) { uint64_t v; if (canon((const uint8_t*)r.blob.data() + p, 0, k, &v)) { o.s.insert(v); o.positions++; } }
    return o;
}
static std::string random_seq(uint32_t n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() % 4]; return s; }

// an index in an allocation of exactly index_bytes, checked against the host's set
struct Index { Dev* d = nullptr; size_t bytes = 0; uint32_t k = 0; Set set; ~Index() { delete d; } };
static int build(rfq_ctx* ctx, const char* what, const Refs& r, uint32_t k, Index* ix) {
    Dev db(ctx, r.blob.data(), r.blob.size()), dof(ctx, r.off.data(), r.off.size() * 8);
    rfq_screen_build_args a; memset(&a, 0, sizeof a);
    a.k = k; a.d_refs = r.blob.empty() ? nullptr : db.p; a.refs_len = r.blob.size(); a.d_ref_off = (const uint64_t*)dof.p; a.n_refs = r.off.size() - 1; a.size_only = 1;
    rfq_screen_build_result q, g;
    if (rfq_screen_build(ctx, &a, &q)) return fail(what, rfq_last_error(ctx));
    uint64_t S = 1024; while (S < 2 * r.blob.size()) S *= 2;
    if (q.slots != S || q.index_bytes != 64 + 8 * S) return fail(what, "the size query differs from the host's");
    delete ix->d; ix->d = new Dev(ctx, nullptr, q.index_bytes); ix->bytes = q.index_bytes; ix->k = k; ix->set = set_of(r, k);
    a.size_only = 0; a.d_index = ix->d->p; a.index_cap = ix->bytes;
    if (a.n_refs == 0) { a.d_refs = nullptr; a.d_ref_off = nullptr; }
    for (int twice = 0; twice < 2; twice++) {
        if (rfq_screen_build(ctx, &a, &g)) return fail(what, rfq_last_error(ctx));
        if (g.n_refs != a.n_refs || g.ref_bases != r.blob.size() || g.n_positions != ix->set.positions || g.n_kmers != ix->set.s.size() || g.slots != S || g.index_bytes != ix->bytes)
            return fail(what, "the build's counts differ from the host's");
    }
    return 0;
}

struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, cand; std::vector<int32_t> lens; };
// n rows of stride L: random reads of 0 .. L bases with pieces of the references in every third, an "other" byte here and there, noise behind the reads
static Rows make_rows(uint32_t n, uint32_t L, int codes, bool mask, const Refs& r) {
    Rows o; o.n = n; o.L = L; o.codes = codes; o.B.resize((size_t)n * L); o.lens.resize(n); if (mask) o.cand.resize(n);
    for (uint32_t g = 0; g < n; g++) {
        const uint32_t l = g % 4 == 0 ? L : rnd() % (L + 1); o.lens[g] = (int32_t)l;
        std::string s = random_seq(L);
        if (g % 3 == 0 && !r.blob.empty()) for (uint32_t at = rnd() % 40; at < l; at += 64 + rnd() % 200) {
            const uint32_t m = std::min<uint32_t>({ 20 + rnd() % 60, l - at, (uint32_t)r.blob.size() }), from = rnd() % (r.blob.size() - m + 1);
            s.replace(at, m, r.blob.substr(from, m));
        }
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
struct Ref { std::vector<uint32_t> kmers, hits; std::vector<uint8_t> keep; rfq_screen_rows_result s; };
static Ref reference(const Rows& r, const Index& ix, const rfq_screen_rows_args& a) {
    const uint32_t nr = a.pairs ? 2 : 1, U = r.n / nr, k = ix.k;
    Ref o; o.kmers.assign(r.n, 0); o.hits.assign(r.n, 0); o.keep.assign(r.n, 0); memset(&o.s, 0, sizeof o.s); o.s.n_units = U;
    for (uint32_t u = 0; u < U; u++) {
        bool cand = true; uint64_t K = 0, H = 0, bases = 0;
        for (uint32_t i = 0; i < nr; i++) if (!r.cand.empty() && !r.cand[nr * u + i]) cand = false;
        if (!cand) continue;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * u + i, l = (uint32_t)r.lens[g];
            for (uint32_t p = 0; p + k <= l; p++) { uint64_t v; if (canon(&r.B[(size_t)g * r.L + p], r.codes, k, &v)) { o.kmers[g]++; o.hits[g] += ix.set.s.count(v) ? 1 : 0; } }
            K += o.kmers[g]; H += o.hits[g]; bases += l;
        }
        const bool matched = H >= std::max(a.min_hits, 1u) && 100 * H >= (uint64_t)a.min_pct * K, keep = a.mode == RFQ_SCREEN_KEEP_MATCHED ? matched : !matched;
        for (uint32_t i = 0; i < nr; i++) o.keep[nr * u + i] = keep;
        o.s.n_candidates++; o.s.n_matched += matched; o.s.n_kept += keep; o.s.kmers += K; o.s.hits += H; o.s.bases_in += bases; o.s.bases_kept += keep ? bases : 0;
    }
    return o;
}
static rfq_screen_rows_args args(int pairs, int mode, uint32_t min_hits, uint32_t min_pct, const Index& ix) {
    rfq_screen_rows_args a; memset(&a, 0, sizeof a); a.pairs = pairs; a.mode = mode; a.min_hits = min_hits; a.min_pct = min_pct; a.d_index = ix.d->p; a.index_bytes = ix.bytes; return a;
}
// outs: bits 1 kmers, 2 hits, 4 keep
static int run(rfq_ctx* ctx, const char* what, const Rows& r, const Index& ix, rfq_screen_rows_args a, int outs, size_t shift) {
    const uint32_t n = r.n; const Ref e = reference(r, ix, a);
    Dev db(ctx, r.B.data(), r.B.size(), shift), dl(ctx, r.lens.data(), n * 4ull), dc(ctx, r.cand.data(), r.cand.size());
    Dev ok(ctx, nullptr, n * 4ull), oh(ctx, nullptr, n * 4ull), okeep(ctx, nullptr, n);
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, nullptr, dl);
    a.d_in = r.cand.empty() ? nullptr : dc.p;
    a.d_kmers = (outs & 1) ? (uint32_t*)ok.p : nullptr; a.d_hits = (outs & 2) ? (uint32_t*)oh.p : nullptr; a.d_keep = (outs & 4) ? okeep.p : nullptr;
    rfq_screen_rows_result g;
    if (rfq_screen_rows(ctx, &in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &e.s, sizeof g)) return fail(what, "the summary differs from the host's");
    std::vector<uint32_t> hk(n + 1), hh(n + 1); std::vector<uint8_t> hp(n + 1);
    if ((outs & 1) && n) { rfq_copy_d2h(ctx, hk.data(), ok.p, n * 4ull); if (memcmp(hk.data(), e.kmers.data(), n * 4ull)) return fail(what, "kmers differ"); }
    if ((outs & 2) && n) { rfq_copy_d2h(ctx, hh.data(), oh.p, n * 4ull); if (memcmp(hh.data(), e.hits.data(), n * 4ull)) return fail(what, "hits differ"); }
    if ((outs & 4) && n) { rfq_copy_d2h(ctx, hp.data(), okeep.p, n); if (memcmp(hp.data(), e.keep.data(), n)) return fail(what, "keep differs"); }
    return 0;
}

static Refs good_refs; static Index good_ix;
static int good(rfq_ctx* ctx) {
    Index fresh;
    if (build(ctx, "a good build after a refusal", good_refs, 16, &fresh)) return 1;
    const Rows r = make_rows(60, 48, 0, true, good_refs);
    return run(ctx, "a good call after a refusal", r, fresh, args(1, RFQ_SCREEN_DROP_MATCHED, 1, 0, fresh), 7, 0) | run(ctx, "the kept index after a refusal", r, good_ix, args(0, 1, 2, 5, good_ix), 7, 1);
}
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_screen_rows_args& a, int code, const char* needle) {
    rfq_screen_rows_result g;
    if (rfq_screen_rows(ctx, &in, &a, &g) != code) return fail(what, "not refused with the expected code");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}
static int build_refused(rfq_ctx* ctx, const char* what, const rfq_screen_build_args& a, int code, const char* needle) {
    rfq_screen_build_result g;
    if (rfq_screen_build(ctx, &a, &g) != code) return fail(what, "not refused with the expected code");
    if (needle && !strstr(rfq_last_error(ctx), needle)) return fail(what, rfq_last_error(ctx));
    return good(ctx);
}

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, builds = 0, refusals = 0;
    good_refs.add(random_seq(90)); good_refs.add(random_seq(20));
    if (build(ctx, "the kept index", good_refs, 16, &good_ix)) return 1;
    // the references: a small set (the slots fit the LDS) and a large one (device memory), with duplicates, a reverse complement, an N, lower case, short and empty ones
    Refs small, large, none, shorts;
    { const std::string x = random_seq(300), y = random_seq(200); std::string rc(x.rbegin(), x.rend()); for (auto& c : rc) c = "TGCA"[strchr("ACGT", c) - "ACGT"];
      std::string lo = y; for (auto& c : lo) c = (char)(c | 0x20); std::string wn = random_seq(120); wn[60] = 'N';
      for (const std::string& s : { x, y, x, rc, lo, wn, std::string(), x.substr(0, 3) }) small.add(s);
      large.add(random_seq(8193)); large.add(x);
      shorts.add(x.substr(0, 3)); shorts.add(std::string()); }
    const uint32_t ks[] = { 4, 15, 16, 17, 25, 31 }, lens[] = { 15, 16, 17, 48, 150, 255, 256, 257, 300, 1023, 1024, 1025, 2080 }, rows[] = { 2, 62, 66, 130 }; const size_t shifts[] = { 0, 1, 7, 15 };
    uint32_t c = 0;
    for (int opt = 0; opt < 3 && !bad; opt++) {                              // the index built under default, general, collide
        const char* const ov[] = { nullptr, "general", "collide" };
        for (const Refs* rf : { &small, &large, &none, &shorts }) for (uint32_t k : ks) {
            if ((c++ + opt) % 3 && rf != &small) continue;                   // (every k with the small set, a third of them with the others)
            if (rfq_set_option(ctx, "RFQ_SCREEN", ov[opt])) return fail("RFQ_SCREEN", rfq_last_error(ctx));
            Index ix; char what[200]; snprintf(what, sizeof what, "build under %s, k %u, %zu reference bytes", ov[opt] ? ov[opt] : "default", k, rf->blob.size());
            bad |= build(ctx, what, *rf, k, &ix); builds++;
            rfq_set_option(ctx, "RFQ_SCREEN", nullptr);
            if (bad) break;
            uint32_t j = c;
            for (uint32_t L : lens) for (int pairs = 0; pairs < 2; pairs++, j++) {
                if (j % 4 != 0 && !(rf == &small && k == 17 && opt == 0)) continue;        // (every stride with one index, a quarter of them with the others)
                const int general = (j / 4) % 2, codes = (j / 8) % 2, mode = (j / 2) % 2; const uint32_t n = L > 1024 ? 10 : rows[j % 4];
                const Rows r = make_rows(n, L, codes, j % 3 == 1, *rf);
                snprintf(what, sizeof what, "index under %s k %u of %zu bytes, general %d row_len %u pairs %d mode %d codes %d rows %u shift %zu", ov[opt] ? ov[opt] : "default", k,
                         rf->blob.size(), general, L, pairs, mode, codes, n, shifts[j % 4]);
                rfq_set_option(ctx, "RFQ_SCREEN", general ? "general" : nullptr);
                bad |= run(ctx, what, r, ix, args(pairs, mode, j % 5, (j % 7) * 3, ix), 7, shifts[j % 4]); calls++;
                rfq_set_option(ctx, "RFQ_SCREEN", nullptr);
            }
            if (rf == &small && k == 16) {
                const Rows r = make_rows(100, 150, 0, false, *rf);
                for (int outs : { 1, 2, 4, 0 }) { bad |= run(ctx, "one output alone", r, ix, args(1, 0, 1, 0, ix), outs, 3); calls++; }
                for (uint32_t n : { 0u, 1u, 2u }) { const Rows z = make_rows(n, 16, 0, false, *rf); bad |= run(ctx, "0, 1, 2 rows", z, ix, args(0, 0, 1, 0, ix), 7, 0); calls++; }
            }
        }
    }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 32, 0, true, good_refs);
        std::vector<int32_t> lp = r.lens; lp.push_back(0);                   // (a word more: the misaligned d_lens stays inside it)
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, lp.data(), 160 + 4), dc(ctx, r.cand.data(), 40), out(ctx, nullptr, 16384);
        const rfq_rows_in in = rows_in(40, 32, 0, db, nullptr, dl);
        const Index& ix = good_ix;
        rfq_screen_rows_args a; rfq_rows_in x;
        a = args(2, 0, 1, 0, ix); bad |= refused(ctx, "pairs 2", in, a, RFQ_E_ARG, "pairs"); refusals++;
        a = args(1, 0, 1, 0, ix); x = in; x.n_rows = 39; bad |= refused(ctx, "an odd n_rows with pairs", x, a, RFQ_E_ARG, "in pairs"); refusals++;
        a = args(0, 2, 1, 0, ix); bad |= refused(ctx, "unknown mode", in, a, RFQ_E_ARG, "mode"); refusals++;
        a = args(0, 0, 1, 101, ix); bad |= refused(ctx, "min_pct 101", in, a, RFQ_E_ARG, "min_pct"); refusals++;
        a = args(0, 0, 1, 0, ix); x = in; x.base_mode = 7; bad |= refused(ctx, "a bad base_mode", x, a, RFQ_E_ARG, "base_mode"); refusals++;
        x = in; x.row_len = 0; bad |= refused(ctx, "row_len 0", x, a, RFQ_E_ARG, "row_len"); refusals++;
        x = in; x.d_bases = nullptr; bad |= refused(ctx, "null d_bases", x, a, RFQ_E_ARG, "null"); refusals++;
        x = in; x.d_lens = nullptr; bad |= refused(ctx, "null d_lens", x, a, RFQ_E_ARG, "null"); refusals++;
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= refused(ctx, "misaligned d_lens", x, a, RFQ_E_ARG, "aligned"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_index = nullptr; bad |= refused(ctx, "null index", in, a, RFQ_E_ARG, "d_index"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_index = ix.d->p + 8; a.index_bytes -= 8; bad |= refused(ctx, "misaligned index", in, a, RFQ_E_ARG, "d_index"); refusals++;
        a = args(0, 0, 1, 0, ix); a.index_bytes = 63; bad |= refused(ctx, "index_bytes 63", in, a, RFQ_E_ARG, "d_index"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_kmers = (uint32_t*)(out.p + 2); bad |= refused(ctx, "misaligned d_kmers", in, a, RFQ_E_ARG, "aligned"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_hits = (uint32_t*)(out.p + 1); bad |= refused(ctx, "misaligned d_hits", in, a, RFQ_E_ARG, "aligned"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_keep = db.p + 40 * 32 - 1; bad |= refused(ctx, "keep on bases", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_in = dc.p; a.d_keep = dc.p; bad |= refused(ctx, "keep on d_in", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_hits = (uint32_t*)dl.p; bad |= refused(ctx, "hits on lens", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = args(0, 0, 1, 0, ix); a.d_kmers = (uint32_t*)(ix.d->p + ix.bytes - 4); bad |= refused(ctx, "kmers on the index", in, a, RFQ_E_ARG, "overlaps"); refusals++;
        a = args(0, 0, 1, 0, ix); x = in; x.n_rows = 1ull << 31; x.row_len = 1; bad |= refused(ctx, "2^31 rows", x, a, RFQ_E_ARG, "too many"); refusals++;
        {   // headers rfq_screen_build does not write; a table with no empty slot
            std::vector<uint8_t> img(ix.bytes); rfq_copy_d2h(ctx, img.data(), ix.d->p, ix.bytes);
            struct Edit { size_t word; uint32_t v; const char* needle; } const edits[] = { { 0, 0x12345678u, "header" }, { 2, 2u, "header" }, { 3, 0u, "k" }, { 3, 32u, "k" }, { 4, 1000u, "slot count" },
                                                                                           { 4, 0u, "slot count" }, { 4, 2048u, "slot count" }, { 5, 1u, "slot count" } };
            for (const Edit& e : edits) {
                std::vector<uint8_t> m = img; memcpy(&m[4 * e.word], &e.v, 4);
                Dev dm(ctx, m.data(), m.size());
                a = args(0, 0, 1, 0, ix); a.d_index = dm.p; bad |= refused(ctx, "a header that is not the build's", in, a, RFQ_E_DATA, e.needle); refusals++;
            }
            std::vector<uint8_t> m = img;
            for (uint64_t i = 0; i < 1024; i++) { const uint64_t v = (1ull << 63) | (1ull << 40) | i; memcpy(&m[64 + 8 * i], &v, 8); }
            Dev dm(ctx, m.data(), m.size());
            for (int general = 0; general < 2; general++) {
                rfq_set_option(ctx, "RFQ_SCREEN", general ? "general" : nullptr);
                a = args(0, 0, 1, 0, ix); a.d_index = dm.p; rfq_screen_rows_result g;
                if (rfq_screen_rows(ctx, &in, &a, &g) != RFQ_OK) bad |= fail("a full index", rfq_last_error(ctx));      // (every probe walks all S slots: the call comes back)
                else if (g.hits != 0 || g.kmers == 0) bad |= fail("a full index", "hits among slots that hold no k-mer of the rows");
                calls++;
            }
            rfq_set_option(ctx, "RFQ_SCREEN", nullptr);
            // headers that pass every check with FEWER slots than the build makes, with the collide flag (the start slot is four bits of the value) and without,
            // in an allocation that ends with the S slots: every slot holds a 4-mer, exactly those hit, nothing behind the slots is read
            for (uint32_t S : { 1u, 2u, 4u, 8u, 16u }) for (uint32_t flags : { 1u, 0u }) for (int general = 0; general < 2 && !bad; general++) {
                Index tiny; tiny.k = 4; tiny.bytes = 64 + 8 * S;
                std::vector<uint8_t> t(tiny.bytes); memcpy(t.data(), img.data(), 64);
                const uint32_t k4 = 4; const uint64_t S64 = S; memcpy(&t[12], &k4, 4); memcpy(&t[16], &S64, 8); memcpy(&t[32], &flags, 4);
                for (uint64_t i = 0; i < S; i++) { const uint64_t v = 15 - i, key = (1ull << 63) | v; tiny.set.s.insert(v); memcpy(&t[64 + 8 * i], &key, 8); }
                tiny.d = new Dev(ctx, t.data(), t.size());
                char what[96]; snprintf(what, sizeof what, "a header of %u slots, flags %u, general %d", S, flags, general);
                rfq_set_option(ctx, "RFQ_SCREEN", general ? "general" : nullptr);
                bad |= run(ctx, what, r, tiny, args(0, 0, 1, 0, tiny), 7, 1); calls++;
                rfq_set_option(ctx, "RFQ_SCREEN", nullptr);
            }
        }
        for (int general = 0; general < 2; general++) for (int pairs = 0; pairs < 2; pairs++) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 20u, 21u, 39u }) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 160); x = in; x.d_lens = (const int32_t*)d2.p;
            a = args(pairs, 0, 1, 0, ix); a.d_in = (row & 1) ? dc.p : nullptr; a.d_kmers = (uint32_t*)out.p; a.d_hits = (uint32_t*)(out.p + 1024); a.d_keep = out.p + 4096;
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_SCREEN", general ? "general" : nullptr);
            rfq_screen_rows_result g;
            if (rfq_screen_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_SCREEN", nullptr);
            bad |= good(ctx); refusals++;
        }
        // the build's refusals
        Refs rr; rr.add(random_seq(50)); rr.add(random_seq(30)); rr.add(random_seq(20));
        std::vector<uint64_t> op = rr.off; op.push_back(0);
        Dev rb(ctx, rr.blob.data(), 100), ro(ctx, op.data(), 40), idx(ctx, nullptr, 64 + 8 * 1024);
        rfq_screen_build_args b0; memset(&b0, 0, sizeof b0); b0.k = 16; b0.d_refs = rb.p; b0.refs_len = 100; b0.d_ref_off = (const uint64_t*)ro.p; b0.n_refs = 3; b0.d_index = idx.p; b0.index_cap = 64 + 8 * 1024;
        rfq_screen_build_args b;
        b = b0; b.k = 3; bad |= build_refused(ctx, "k 3", b, RFQ_E_ARG, "k must be"); refusals++;
        b = b0; b.k = 32; b.size_only = 1; bad |= build_refused(ctx, "k 32", b, RFQ_E_ARG, "k must be"); refusals++;
        b = b0; b.d_refs = nullptr; bad |= build_refused(ctx, "null d_refs", b, RFQ_E_ARG, "null"); refusals++;
        b = b0; b.d_ref_off = nullptr; bad |= build_refused(ctx, "null d_ref_off", b, RFQ_E_ARG, "null"); refusals++;
        b = b0; b.d_ref_off = (const uint64_t*)(ro.p + 4); b.n_refs = 2; bad |= build_refused(ctx, "misaligned d_ref_off", b, RFQ_E_ARG, "8-byte"); refusals++;
        b = b0; b.d_index = idx.p + 8; bad |= build_refused(ctx, "misaligned d_index", b, RFQ_E_ARG, "16-byte"); refusals++;
        b = b0; b.d_index = nullptr; bad |= build_refused(ctx, "null d_index", b, RFQ_E_ARG, "null d_index"); refusals++;
        b = b0; b.index_cap -= 1; bad |= build_refused(ctx, "an index buffer one byte short", b, RFQ_E_NOSPACE, "need 8256 bytes"); refusals++;
        for (int which = 0; which < 3; which++) {
            std::vector<uint64_t> o2 = rr.off; const char* needle = "first such reference: 1)";
            if (which == 0) o2[2] = 40; else if (which == 1) { o2[3] = 101; needle = "first such reference: 2)"; } else { o2[0] = ~0ull; needle = "first such reference: 0)"; }
            Dev r2(ctx, o2.data(), 32); b = b0; b.d_ref_off = (const uint64_t*)r2.p;
            bad |= build_refused(ctx, "offsets that decrease or end past refs_len", b, RFQ_E_ARG, needle); refusals++;
        }
        if (rfq_set_option(ctx, "RFQ_SCREEN", "staged") != RFQ_E_ARG) bad |= fail("RFQ_SCREEN=staged", "not refused");
    }
    delete good_ix.d; good_ix.d = nullptr;
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("screen_asan: %d builds (k 4 .. 31; a set that fits the LDS, one that does not, none, only short references; under default / general / collide, each twice) and %d good calls (13 row strides x rows / pairs x 2 modes x 2 base modes at shifts 0 / 1 / 7 / 15, both kernels' paths, outputs alone, 0 / 1 / 2 rows, a full index, headers of 1 .. 16 slots with and without the collide flag), %d refusals (19 + 8 on the host, 8 bad headers, 32 + 3 on the device) each followed by a good build and two good calls: all as the host reference says, no sanitizer report\n", builds, calls, refusals);
    return 0;
}
