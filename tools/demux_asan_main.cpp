// demux_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_demux_rows on the SIMT-interpreter build (CPU only, no Python): tools/demux_asan.sh
// compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   demux_asan_main         good shapes of tests/_demux.py - barcodes of 1 .. 32 bases at offsets 0 .. 40, row strides 16 .. 1040, both base modes, a mask, buffer
//   shifts 0 / 1 / 5 / 15, one set and two, every combination and a sample sheet, 4096 barcodes, counts in LDS and in device memory, calls of more units than one
//   step of the grid, the default path and
//   RFQ_DEMUX=general - with rows in allocations that end where their data ends and outputs of exactly the bytes a call may write, compared with a host loop over
//   units, barcodes and positions written from include/rfq_hip.h; then every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <set>
#include <string>
#include <vector>

static uint32_t cls_of(int codes, uint8_t c) {
    if (codes) return c < 4 ? c : 4;
    switch (c & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}
static std::string random_seq(uint32_t n) { std::string s(n, 'A'); for (auto& c : s) c = "ACGT"[rnd() % 4]; return s; }
// n distinct barcodes of len bases, [n][len]
static std::string make_set(uint32_t n, uint32_t len) {
    std::set<std::string> seen; std::string out;
    while (seen.size() < n) { const std::string s = random_seq(len); if (seen.insert(s).second) out += s; }
    return out;
}
struct Rows { uint32_t n = 0, L = 1; int codes = 0; std::vector<uint8_t> B, cand; std::vector<int32_t> lens; };
struct Call {
    int pairs = 0; uint32_t n[2] = { 0, 0 }, len[2] = { 0, 0 }, off[2] = { 0, 0 }, skip[2] = { 0, 0 }; std::string bc[2]; std::vector<int32_t> sheet; bool has_sheet = false;
    uint32_t max_mm = 1, min_delta = 1;
    uint32_t n_samples() const { return !n[1] ? n[0] : (has_sheet ? (uint32_t)(sheet.size() / 2) : n[0] * n[1]); }
};
// n rows of stride L: random reads of 0 .. L bases, most with a barcode of their set planted (exact, one or two mismatches, an N, lower case), noise behind the reads
static Rows make_rows(uint32_t n, uint32_t L, int codes, bool mask, const Call& c) {
    Rows o; o.n = n; o.L = L; o.codes = codes; o.B.resize((size_t)n * L); o.lens.resize(n); if (mask) o.cand.resize(n);
    for (uint32_t g = 0; g < n; g++) {
        const uint32_t i = c.pairs ? g & 1u : 0u, need = c.off[i] + c.len[i];
        const uint32_t l = g % 5 == 4 ? rnd() % (L + 1) : (need <= L ? need + rnd() % (L - need + 1) : L); o.lens[g] = (int32_t)l;
        std::string s = random_seq(L);
        if (c.n[i] && need <= L && g % 7 != 6) {
            std::string b = c.bc[i].substr((size_t)(rnd() % c.n[i]) * c.len[i], c.len[i]);
            if (g % 3 == 1) b[rnd() % c.len[i]] = "ACGT"[rnd() % 4];
            if (g % 11 == 2) b[rnd() % c.len[i]] = 'N';
            if (g % 13 == 3) for (auto& ch : b) ch = (char)(ch | 0x20);
            s.replace(c.off[i], c.len[i], b);
        }
        for (uint32_t j = 0; j < L; j++) {
            uint8_t b = (uint8_t)s[j];
            if (codes) b = (uint8_t)(cls_of(0, b) < 4 ? cls_of(0, b) : 4 + rnd() % 250);
            o.B[(size_t)g * L + j] = j < l ? b : (uint8_t)rnd();
        }
        if (mask) o.cand[g] = rnd() % 6 ? (uint8_t)(1 + rnd() % 255) : 0;
    }
    return o;
}
struct Want { std::vector<int32_t> sample, best, start; std::vector<uint8_t> why, dist, keep; std::vector<uint64_t> counts; rfq_demux_rows_result r; };
static Want model(const Rows& r, const Call& c) {
    const uint32_t nr = c.pairs ? 2 : 1, U = r.n / nr, ns = c.n_samples();
    Want w; w.sample.assign(U, -1); w.why.assign(U, 0); w.best.assign(r.n, -1); w.dist.assign(r.n, 255); w.keep.assign(r.n, 0); w.start.assign(r.n, 0); w.counts.assign(ns + 1, 0);
    memset(&w.r, 0, sizeof w.r); w.r.n_units = U; w.r.n_samples = ns;
    std::vector<int32_t> table;
    if (c.has_sheet) { table.assign((size_t)c.n[0] * c.n[1], -1); for (uint32_t s = 0; s < ns; s++) table[(size_t)c.sheet[2 * s] * c.n[1] + c.sheet[2 * s + 1]] = (int32_t)s; }
    for (uint32_t u = 0; u < U; u++) {
        bool cand = true;
        for (uint32_t i = 0; i < nr; i++) if (!r.cand.empty() && !r.cand[nr * u + i]) cand = false;
        if (!cand) { w.why[u] = RFQ_DEMUX_MASKED; continue; }
        w.r.n_candidates++;
        uint32_t why = 0; bool exact = true;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * u + i, l = (uint32_t)r.lens[g];
            w.r.bases_in += l;
            if (!c.n[i]) continue;
            if (l < c.off[i] + c.len[i]) { why |= RFQ_DEMUX_SHORT; continue; }
            uint32_t d1 = c.len[i] + 1, d2 = c.len[i] + 1, best = 0;
            for (uint32_t k = 0; k < c.n[i]; k++) {
                uint32_t d = 0;
                for (uint32_t j = 0; j < c.len[i]; j++) { const uint32_t x = cls_of(r.codes, r.B[(size_t)g * r.L + c.off[i] + j]); if (x > 3 || x != cls_of(0, (uint8_t)c.bc[i][(size_t)k * c.len[i] + j])) d++; }
                if (d < d1) { d2 = d1; d1 = d; best = k; } else if (d < d2) d2 = d;
            }
            w.best[g] = (int32_t)best; w.dist[g] = (uint8_t)d1; exact = exact && d1 == 0;
            why |= d1 > c.max_mm ? RFQ_DEMUX_NONE : (d2 - d1 < c.min_delta ? RFQ_DEMUX_AMBIG : 0);
        }
        int32_t sample = -1;
        if (!why) {
            if (!c.n[1]) sample = w.best[nr * u];
            else { const size_t at = (size_t)w.best[2 * u] * c.n[1] + w.best[2 * u + 1]; sample = c.has_sheet ? table[at] : (int32_t)at; if (sample < 0) why = RFQ_DEMUX_COMBO; }
        }
        w.why[u] = (uint8_t)why;
        w.r.why_none += !!(why & RFQ_DEMUX_NONE); w.r.why_ambig += !!(why & RFQ_DEMUX_AMBIG); w.r.why_short += !!(why & RFQ_DEMUX_SHORT); w.r.why_combo += !!(why & RFQ_DEMUX_COMBO);
        if (why) { w.counts[ns]++; continue; }
        w.sample[u] = sample; w.counts[sample]++; w.r.n_assigned++; w.r.n_exact += exact;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * u + i, l = (uint32_t)r.lens[g];
            w.keep[g] = 1;
            if (c.n[i]) w.start[g] = (int32_t)std::min(l, c.off[i] + c.len[i] + c.skip[i]);
            w.r.bases_out += l - (uint32_t)w.start[g];
        }
    }
    return w;
}
static rfq_demux_rows_args args_of(const Call& c) {
    rfq_demux_rows_args a; memset(&a, 0, sizeof a);
    a.pairs = c.pairs; a.n1 = c.n[0]; a.len1 = c.len[0]; a.off1 = c.off[0]; a.skip1 = c.skip[0]; a.h_bc1 = (const uint8_t*)c.bc[0].data();
    if (c.n[1]) { a.n2 = c.n[1]; a.len2 = c.len[1]; a.off2 = c.off[1]; a.skip2 = c.skip[1]; a.h_bc2 = (const uint8_t*)c.bc[1].data(); }
    if (c.has_sheet) { a.h_pairs = c.sheet.data(); a.n_samples = (uint32_t)(c.sheet.size() / 2); }
    a.max_mm = c.max_mm; a.min_delta = c.min_delta;
    return a;
}
// one call into buffers of exactly the bytes it may write (each ends where its allocation ends), on both formulations, against the model
static int check(rfq_ctx* ctx, const char* what, const Rows& r, const Call& c, size_t shift, int* calls) {
    const Want w = model(r, c);
    const uint32_t n = r.n, U = n / (c.pairs ? 2 : 1), ns = c.n_samples();
    Dev db(ctx, r.B.data(), r.B.size(), shift), dl(ctx, r.lens.data(), n * 4ull), dc(ctx, r.cand.data(), r.cand.size());
    const rfq_rows_in in = rows_in(n, r.L, r.codes, db, nullptr, dl);
    for (const char* o : { (const char*)nullptr, "general" }) {
        Dev os(ctx, nullptr, U * 4ull), ow(ctx, nullptr, U), ob(ctx, nullptr, n * 4ull), od(ctx, nullptr, n), ok(ctx, nullptr, n), ot(ctx, nullptr, n * 4ull), oc(ctx, nullptr, (ns + 1) * 8ull);
        rfq_demux_rows_args a = args_of(c);
        a.d_in = r.cand.empty() ? nullptr : dc.p; a.d_sample = (int32_t*)os.p; a.d_why = ow.p; a.d_best = (int32_t*)ob.p; a.d_dist = od.p; a.d_keep = ok.p; a.d_start = (int32_t*)ot.p;
        a.d_counts = (uint64_t*)oc.p;
        rfq_demux_rows_result g;
        rfq_set_option(ctx, "RFQ_DEMUX", o);
        const int rc = rfq_demux_rows(ctx, &in, &a, &g);
        rfq_set_option(ctx, "RFQ_DEMUX", nullptr);
        if (rc) return fail(what, rfq_last_error(ctx));
        if (memcmp(&g, &w.r, sizeof g)) return fail(what, "the result differs from the host's");
        std::vector<int32_t> hs(U + 1), hb(n + 1), ht(n + 1); std::vector<uint8_t> hw(U + 1), hd(n + 1), hk(n + 1); std::vector<uint64_t> hc(ns + 1);
        if (n) { rfq_copy_d2h(ctx, hs.data(), os.p, U * 4ull); rfq_copy_d2h(ctx, hw.data(), ow.p, U); rfq_copy_d2h(ctx, hb.data(), ob.p, n * 4ull); rfq_copy_d2h(ctx, hd.data(), od.p, n);
                 rfq_copy_d2h(ctx, hk.data(), ok.p, n); rfq_copy_d2h(ctx, ht.data(), ot.p, n * 4ull); }
        rfq_copy_d2h(ctx, hc.data(), oc.p, (ns + 1) * 8ull);
        if (n && (memcmp(hs.data(), w.sample.data(), U * 4ull) || memcmp(hw.data(), w.why.data(), U))) return fail(what, "sample or why differ");
        if (n && (memcmp(hb.data(), w.best.data(), n * 4ull) || memcmp(hd.data(), w.dist.data(), n))) return fail(what, "best or dist differ");
        if (n && (memcmp(hk.data(), w.keep.data(), n) || memcmp(ht.data(), w.start.data(), n * 4ull))) return fail(what, "keep or start differ");
        if (memcmp(hc.data(), w.counts.data(), (ns + 1) * 8ull)) return fail(what, "counts differ");
        ++*calls;
    }
    return 0;
}
static Call one_set(uint32_t n, uint32_t len, uint32_t off, uint32_t skip) { Call c; c.n[0] = n; c.len[0] = len; c.off[0] = off; c.skip[0] = skip; c.bc[0] = make_set(n, len); return c; }
static Call two_sets(uint32_t n1, uint32_t len1, uint32_t off1, uint32_t n2, uint32_t len2, uint32_t off2, uint32_t listed) {
    Call c = one_set(n1, len1, off1, 1); c.pairs = 1; c.n[1] = n2; c.len[1] = len2; c.off[1] = off2; c.skip[1] = 2; c.bc[1] = make_set(n2, len2);
    if (listed) {
        c.has_sheet = true; std::set<uint32_t> seen;
        while (seen.size() < listed) { const uint32_t p = rnd() % (n1 * n2); if (seen.insert(p).second) { c.sheet.push_back((int32_t)(p / n2)); c.sheet.push_back((int32_t)(p % n2)); } }
    }
    return c;
}
static int good(rfq_ctx* ctx) {
    int calls = 0;
    const Call c = two_sets(3, 6, 1, 2, 18, 0, 4);
    return check(ctx, "a good call after a refusal", make_rows(10, 40, 0, false, c), c, 0, &calls);
}
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_demux_rows_args& a, const char* needle) {
    rfq_demux_rows_result g;
    const int rc = rfq_demux_rows(ctx, &in, &a, &g);
    if (rc != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) { fprintf(stderr, "%s: rc %d, \"%s\" (wanted \"%s\")\n", what, rc, rfq_last_error(ctx), needle); return 1; }
    return good(ctx);
}

static const size_t SHIFTS[4] = { 0, 1, 5, 15 };

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, refusals = 0;
    // one set: every length class x offsets across the 16-byte groups x strides of every kernel path, shifts, both modes, masks
    for (uint32_t len : { 1u, 8u, 16u, 17u, 32u }) for (uint32_t off : { 0u, 1u, 15u, 16u, 31u, 40u }) {
        const Call c = one_set(len == 1 ? 4 : 7, len, off, off % 3);
        for (uint32_t L : { off + len, 50u, 160u, 272u }) {
            if (L < off + len || bad) continue;
            const int codes = (int)((len + off + L) & 1u);
            bad |= check(ctx, "one set", make_rows(70, L, codes, (L & 2u) != 0, c), c, SHIFTS[(len + off) % 4], &calls);
        }
    }
    if (!bad) {   // the deltas and one barcode
        Call c = one_set(5, 8, 2, 0);
        c.bc[0].replace(8, 8, c.bc[0].substr(0, 8)); c.bc[0][8 + 3] = c.bc[0][3] == 'A' ? 'C' : 'A';         // barcode 1 is one base from barcode 0
        const Rows r = make_rows(120, 24, 0, false, c);
        for (uint32_t mm = 0; mm < 4 && !bad; mm++) for (uint32_t delta : { 0u, 1u, 2u, 3u, 33u }) { c.max_mm = mm; c.min_delta = delta; bad |= check(ctx, "deltas", r, c, 0, &calls); }
        Call one = one_set(1, 9, 0, 40); one.max_mm = 32;
        for (uint32_t delta : { 0u, 1u, 9u, 10u }) { one.min_delta = delta; bad |= check(ctx, "one barcode", make_rows(30, 16, 1, true, one), one, 1, &calls); }
    }
    if (!bad) {   // pairs: set 1 only, every combination, sample sheets; counts in LDS (8192 cells) and in device memory (8193); 4096 barcodes; long rows; no rows
        Call c = one_set(6, 8, 3, 2); c.pairs = 1;
        bad |= check(ctx, "pairs, set 1 only", make_rows(64, 40, 0, true, c), c, 0, &calls);
        const Call all = two_sets(6, 8, 2, 5, 17, 19, 0), third = two_sets(6, 8, 2, 5, 17, 19, 10);
        bad |= check(ctx, "pairs, every combination", make_rows(200, 64, 1, true, all), all, 5, &calls) | check(ctx, "pairs, a sample sheet", make_rows(200, 64, 0, false, third), third, 0, &calls);
        const Call lds = two_sets(128, 6, 0, 64, 5, 0, 8191), mem = two_sets(128, 6, 0, 64, 5, 0, 8192);
        bad |= check(ctx, "8192 count cells", make_rows(600, 12, 0, false, lds), lds, 0, &calls) | check(ctx, "8193 count cells", make_rows(600, 12, 0, false, mem), mem, 1, &calls);
        const Call many = one_set(4096, 8, 0, 0);
        bad |= check(ctx, "4096 barcodes", make_rows(40, 8, 0, false, many), many, 0, &calls);
        const Call big = two_sets(4096, 17, 0, 200, 32, 5, 0);
        bad |= check(ctx, "4096 x 200 barcodes of two words", make_rows(12, 48, 1, false, big), big, 15, &calls);
        const Call lng = one_set(9, 20, 1010, 3);
        bad |= check(ctx, "rows of 1040", make_rows(9, 1040, 0, false, lng), lng, 1, &calls) | check(ctx, "514 rows", make_rows(514, 16, 0, true, c), c, 0, &calls);
        // more units than one step of the grid takes (the interpreter reports 4 compute units: 4 x 4 x 256 = 4096 units a step): several steps a workgroup, the last part empty
        const Call steps1 = one_set(24, 8, 2, 1);
        bad |= check(ctx, "9001 rows, several steps", make_rows(9001, 16, 0, true, steps1), steps1, 1, &calls) | check(ctx, "4200 pairs, several steps", make_rows(8400, 64, 1, false, third), third, 0, &calls);
        Rows none; none.L = 16;
        bad |= check(ctx, "no rows", none, third, 0, &calls);
    }
    if (!bad) {   // the refusals
        const Call c = two_sets(4, 8, 0, 3, 6, 0, 0);
        const Rows r = make_rows(12, 32, 0, true, c);
        Dev db(ctx, r.B.data(), r.B.size()), dl(ctx, r.lens.data(), 48), dc(ctx, r.cand.data(), 12), out(ctx, nullptr, 16384);
        const rfq_rows_in in = rows_in(12, 32, 0, db, nullptr, dl);
        const rfq_demux_rows_args a0 = args_of(c);
        rfq_demux_rows_args s0 = a0; s0.pairs = 0; s0.n2 = s0.len2 = s0.off2 = s0.skip2 = 0; s0.h_bc2 = nullptr;                   // set 1 alone, rows
        rfq_demux_rows_args a; rfq_rows_in x;
        const int32_t sheet[6] = { 0, 0, 1, 1, 0, 0 };
        a = a0; x = in; x.n_rows = 11; bad |= refused(ctx, "an odd row count", x, a, "rows in pairs"); refusals++;
        a = a0; a.pairs = 2; bad |= refused(ctx, "pairs 2", in, a, "0 or 1"); refusals++;
        a = a0; a.pairs = 0; bad |= refused(ctx, "set 2 without pairs", in, a, "for pairs"); refusals++;
        a = s0; a.skip2 = 1; bad |= refused(ctx, "skip2 without pairs", in, a, "for pairs"); refusals++;
        a = s0; a.off2 = 1; bad |= refused(ctx, "off2 without pairs", in, a, "for pairs"); refusals++;
        a = s0; a.h_pairs = sheet; a.n_samples = 1; bad |= refused(ctx, "a sheet without pairs", in, a, "for pairs"); refusals++;
        a = s0; a.pairs = 1; a.h_pairs = sheet; a.n_samples = 1; bad |= refused(ctx, "a sheet without set 2", in, a, "needs set 2"); refusals++;
        a = s0; a.h_bc1 = nullptr; a.n1 = 0; bad |= refused(ctx, "no set 1", in, a, "no set 1"); refusals++;
        a = s0; a.h_bc1 = nullptr; bad |= refused(ctx, "null h_bc1", in, a, "null h_bc1"); refusals++;
        a = a0; a.h_bc2 = nullptr; bad |= refused(ctx, "null h_bc2", in, a, "null h_bc2"); refusals++;
        a = s0; a.n1 = 0; bad |= refused(ctx, "n1 0", in, a, "number of barcodes"); refusals++;
        a = s0; a.n1 = 4097; bad |= refused(ctx, "n1 4097", in, a, "number of barcodes"); refusals++;
        a = a0; a.n2 = 0; bad |= refused(ctx, "n2 0", in, a, "number of barcodes"); refusals++;
        a = s0; a.len1 = 0; bad |= refused(ctx, "len1 0", in, a, "barcode length"); refusals++;
        a = s0; a.len1 = 33; bad |= refused(ctx, "len1 33", in, a, "barcode length"); refusals++;
        a = a0; a.len2 = 33; bad |= refused(ctx, "len2 33", in, a, "barcode length"); refusals++;
        { const Call big = two_sets(2048, 6, 0, 513, 5, 0, 0); a = args_of(big); bad |= refused(ctx, "n1 * n2 over 2^20", in, a, "2^20"); refusals++; }
        a = s0; a.max_mm = 33; bad |= refused(ctx, "max_mm 33", in, a, "max_mm"); refusals++;
        a = s0; a.min_delta = 34; bad |= refused(ctx, "min_delta 34", in, a, "min_delta"); refusals++;
        a = a0; a.h_pairs = sheet; a.n_samples = 0; bad |= refused(ctx, "an empty sheet", in, a, "n_samples"); refusals++;
        a = a0; a.h_pairs = sheet; a.n_samples = 65537; bad |= refused(ctx, "a sheet of 65537", in, a, "n_samples"); refusals++;
        { std::string b = c.bc[0]; b[11] = 'N'; a = s0; a.h_bc1 = (const uint8_t*)b.data(); bad |= refused(ctx, "an N in a barcode", in, a, "0x4e at 3"); refusals++; }
        { std::string b = c.bc[1]; b[12] = 0; a = a0; a.h_bc2 = (const uint8_t*)b.data(); bad |= refused(ctx, "a NUL in a barcode", in, a, "set 2: barcode 2"); refusals++; }
        { std::string b = c.bc[0]; b.replace(24, 8, b.substr(8, 8)); b[25] = (char)(b[25] | 0x20); a = s0; a.h_bc1 = (const uint8_t*)b.data(); bad |= refused(ctx, "equal barcodes", in, a, "barcodes 1 and 3 are equal"); refusals++; }
        { const int32_t s[4] = { 0, 0, 4, 0 }; a = a0; a.h_pairs = s; a.n_samples = 2; bad |= refused(ctx, "a sheet index out of range", in, a, "pair 1 is (4, 0)"); refusals++; }
        { const int32_t s[2] = { 0, -1 }; a = a0; a.h_pairs = s; a.n_samples = 1; bad |= refused(ctx, "a negative sheet index", in, a, "pair 0 is (0, -1)"); refusals++; }
        a = a0; a.h_pairs = sheet; a.n_samples = 3; bad |= refused(ctx, "a pair listed twice", in, a, "twice"); refusals++;
        a = s0; a.off1 = 0x7FFFFFF8u; bad |= refused(ctx, "off + len + skip at 2^31", in, a, "does not fit"); refusals++;
        a = a0; a.skip2 = 0xFFFFFFFFu; bad |= refused(ctx, "skip2 2^32 - 1", in, a, "does not fit"); refusals++;
        a = s0; x = in; x.base_mode = 7; bad |= refused(ctx, "a bad base_mode", x, a, "base_mode"); refusals++;
        x = in; x.row_len = 0; bad |= refused(ctx, "row_len 0", x, a, "row_len"); refusals++;
        x = in; x.d_bases = nullptr; bad |= refused(ctx, "null d_bases", x, a, "null"); refusals++;
        x = in; x.d_lens = nullptr; bad |= refused(ctx, "null d_lens", x, a, "null"); refusals++;
        x = in; x.d_lens = (const int32_t*)(dl.p + 2); bad |= refused(ctx, "misaligned d_lens", x, a, "aligned"); refusals++;
        a = s0; a.d_sample = (int32_t*)(out.p + 2); bad |= refused(ctx, "misaligned d_sample", in, a, "4-byte"); refusals++;
        a = s0; a.d_best = (int32_t*)(out.p + 1); bad |= refused(ctx, "misaligned d_best", in, a, "4-byte"); refusals++;
        a = s0; a.d_start = (int32_t*)(out.p + 3); bad |= refused(ctx, "misaligned d_start", in, a, "4-byte"); refusals++;
        a = s0; a.d_counts = (uint64_t*)(out.p + 4); bad |= refused(ctx, "misaligned d_counts", in, a, "8-byte"); refusals++;
        a = s0; a.d_keep = db.p + 12 * 32 - 1; bad |= refused(ctx, "keep on bases", in, a, "overlaps the input"); refusals++;
        a = s0; a.d_in = dc.p; a.d_why = dc.p + 11; bad |= refused(ctx, "why on d_in", in, a, "overlaps the input d_in"); refusals++;
        a = s0; a.d_start = (int32_t*)dl.p; bad |= refused(ctx, "start on lens", in, a, "overlaps the input"); refusals++;
        a = s0; a.d_sample = (int32_t*)out.p; a.d_why = out.p + 47; bad |= refused(ctx, "why on sample", in, a, "overlaps the output"); refusals++;
        a = s0; a.d_dist = out.p + 32; a.d_counts = (uint64_t*)out.p; bad |= refused(ctx, "dist on counts", in, a, "overlaps the output"); refusals++;
        a = s0; x = in; x.n_rows = 1ull << 31; x.row_len = 1; bad |= refused(ctx, "2^31 rows", x, a, "too many"); refusals++;
        for (const char* o : { (const char*)nullptr, "general" }) for (int32_t v : { -1, 33 }) for (uint32_t row : { 0u, 7u, 11u }) for (int pairs = 0; pairs < 2; pairs++) {
            std::vector<int32_t> l2 = r.lens; l2[row] = v;
            Dev d2(ctx, l2.data(), 48); x = in; x.d_lens = (const int32_t*)d2.p;
            a = pairs ? a0 : s0; a.d_in = (row & 1) ? dc.p : nullptr; a.d_best = (int32_t*)out.p;
            char needle[64]; snprintf(needle, sizeof needle, "first such row: %u)", row);
            rfq_set_option(ctx, "RFQ_DEMUX", o);
            rfq_demux_rows_result g;
            if (rfq_demux_rows(ctx, &x, &a, &g) != RFQ_E_ARG || !strstr(rfq_last_error(ctx), needle)) bad |= fail("a bad length", rfq_last_error(ctx));
            rfq_set_option(ctx, "RFQ_DEMUX", nullptr);
            bad |= good(ctx); refusals++;
        }
        if (rfq_set_option(ctx, "RFQ_DEMUX", "collide") != RFQ_E_ARG) bad |= fail("RFQ_DEMUX=collide", "not refused");
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("demux_asan: %d good calls (barcodes of 1 .. 32 bases at offsets 0 .. 40, strides 16 .. 1040, both base modes, masks, shifts 0 / 1 / 5 / 15, one set and two, sheets, "
           "4096 barcodes, counts in LDS and in device memory, default / general) and %d refusals (host and device) each followed by a good call: all as the host loop says, "
           "no sanitizer report\n", calls, refusals);
    return 0;
}
