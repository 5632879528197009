// group_asan_main.cpp - stand-alone host program for a sanitizer run of rfq_group_rows on the SIMT-interpreter build (CPU only, no Python): tools/group_asan.sh
// compiles it with the library's sources under -fsanitize=address,undefined and runs it.
//   group_asan_main         good shapes of tests/_group.py - unit counts around a wave, a workgroup's step and a tile of the sort (GR_TILE = 2048), totals of 1 .. 65536
//   bins on both sides of the one-pass / two-pass seam, the bin patterns, the rest bin kept and dropped, rows and pairs, masks, windows and min_len, rows with and
//   without names, buffer shifts 0 / 1 / 5 / 15, strides that are and are not multiples of 16, every subset of outputs that matters - with rows in allocations that
//   end where their data ends and outputs of exactly the bytes a call may write, compared with a host loop (who stays, a stable sort of the kept units by bin, the
//   rows' own bytes) written from include/rfq_hip.h; then every refusal, each followed by a good call.  Anything unexpected is an error (exit 1).
#include "asan_common.h"
#include <algorithm>
#include <string>
#include <vector>

struct Rows { uint32_t n = 0, L = 1; bool named = true; std::vector<uint8_t> B, Q, keep; std::vector<int32_t> lens, start, len; std::vector<std::string> names; };
struct Call { std::vector<int32_t> bins; uint32_t n_bins = 1; int rest = 1, pairs = 0; uint32_t min_len = 1; };
// n rows of stride L: random bytes in and behind the reads, reads of 1 .. L bases, distinct names (one of no bytes, one long), part masked, windows that trim 0 .. 2 bases
static Rows make_rows(uint32_t n, uint32_t L, bool named, bool mask, bool window) {
    Rows o; o.n = n; o.L = L; o.named = named; o.B.resize((size_t)n * L); o.Q.resize((size_t)n * L); o.lens.resize(n);
    for (auto& b : o.B) b = (uint8_t)rnd();
    for (auto& b : o.Q) b = (uint8_t)rnd();
    for (uint32_t g = 0; g < n; g++) {
        o.lens[g] = (int32_t)(1 + rnd() % L);
        if (named) { char buf[32]; snprintf(buf, sizeof buf, "@r%u.", g); o.names.push_back(g % 97 == 5 ? std::string() : std::string(buf) + std::string(g % 211 == 7 ? 700 : g % 5, 'x')); }
    }
    if (mask) { o.keep.resize(n); for (auto& k : o.keep) k = rnd() % 7 ? (uint8_t)(1 + rnd() % 255) : 0; }
    if (window) {
        o.start.resize(n); o.len.resize(n);
        for (uint32_t g = 0; g < n; g++) { const int32_t l = o.lens[g], s = (int32_t)(rnd() % 3) % (l + 1); o.start[g] = s; o.len[g] = (l - s) - (int32_t)(rnd() % 2) % (l - s + 1); }
    }
    return o;
}
struct Want { std::vector<uint32_t> idx; std::vector<uint64_t> bin_off, name_off; std::string blob; std::vector<int32_t> lens; rfq_group_rows_result r; };
static Want model(const Rows& r, const Call& c) {
    const uint32_t nr = c.pairs ? 2 : 1, U = r.n / nr, T = c.n_bins + (uint32_t)c.rest;
    Want w; memset(&w.r, 0, sizeof w.r); w.r.n_in = r.n;
    std::vector<int32_t> win_s(r.n), win_l(r.n); std::vector<uint8_t> stand(r.n);
    for (uint32_t g = 0; g < r.n; g++) {
        win_s[g] = r.start.empty() ? 0 : r.start[g]; win_l[g] = r.len.empty() ? r.lens[g] - win_s[g] : r.len[g];
        const bool k = r.keep.empty() || r.keep[g], falls = c.bins[g / nr] < 0 && !c.rest, shrt = (uint32_t)win_l[g] < c.min_len;
        if (!k) w.r.dropped_mask++; else if (falls) w.r.dropped_bin++; else if (shrt) w.r.dropped_short++;
        stand[g] = k && !falls && !shrt;
    }
    std::vector<std::pair<uint32_t, uint32_t>> units;                        // (key, unit)
    for (uint32_t u = 0; u < U; u++) {
        bool all = true; for (uint32_t i = 0; i < nr; i++) all = all && stand[nr * u + i];
        for (uint32_t i = 0; i < nr; i++) if (stand[nr * u + i] && !all) w.r.dropped_mate++;
        if (all) units.push_back({ c.bins[u] < 0 ? c.n_bins : (uint32_t)c.bins[u], u });
    }
    std::stable_sort(units.begin(), units.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
    w.bin_off.assign(T + 1, 0); w.name_off.push_back(0);
    std::vector<uint8_t> used(T, 0);
    for (auto& ku : units) {
        used[ku.first] = 1;
        for (uint32_t b = ku.first + 1; b <= T; b++) w.bin_off[b] += nr;
        for (uint32_t i = 0; i < nr; i++) {
            const uint32_t g = nr * ku.second + i;
            w.idx.push_back(g); w.lens.push_back(win_l[g]); w.r.n_bases += (uint64_t)win_l[g]; w.r.max_len = std::max(w.r.max_len, (uint32_t)win_l[g]);
            if (r.named) { w.blob += r.names[g]; w.name_off.push_back(w.blob.size()); w.r.max_name = std::max(w.r.max_name, (uint32_t)r.names[g].size()); }
        }
    }
    w.r.n_rows = w.idx.size(); w.r.names_len = w.blob.size();
    for (uint8_t x : used) w.r.n_bins_used += x;
    return w;
}
struct DevRows {
    Dev b, q, l, blob, off, keep, start, len, bin; rfq_rows_in in;
    DevRows(rfq_ctx* ctx, const Rows& r, const Call& c, size_t shift, const std::string& names, const std::vector<uint64_t>& noff)
        : b(ctx, r.B.data(), r.B.size(), shift), q(ctx, r.Q.data(), r.Q.size(), shift), l(ctx, r.lens.data(), r.n * 4ull), blob(ctx, names.data(), names.size(), shift),
          off(ctx, noff.data(), noff.size() * 8), keep(ctx, r.keep.data(), r.keep.size()), start(ctx, r.start.data(), r.start.size() * 4), len(ctx, r.len.data(), r.len.size() * 4),
          bin(ctx, c.bins.data(), c.bins.size() * 4) {
        in = rows_in(r.n, r.L, 0, b, &q, l);
        if (r.named) { in.d_names = blob.p; in.names_len = names.size(); in.d_name_off = (const uint64_t*)off.p; }
    }
    rfq_group_rows_args args(const Rows& r, const Call& c) const {
        rfq_group_rows_args a; memset(&a, 0, sizeof a);
        a.d_keep = r.keep.empty() ? nullptr : keep.p; a.d_start = r.start.empty() ? nullptr : (const int32_t*)start.p; a.d_len = r.len.empty() ? nullptr : (const int32_t*)len.p;
        a.pairs = c.pairs; a.min_len = c.min_len; a.d_bin = (const int32_t*)bin.p; a.n_bins = c.n_bins; a.rest = c.rest;
        return a;
    }
};
static void names_of(const Rows& r, std::string* blob, std::vector<uint64_t>* off) {
    off->assign(1, 0);
    for (auto& s : r.names) { *blob += s; off->push_back(blob->size()); }
    if (!r.named) off->clear();
}
static const uint8_t PAD_B = 0xA7, PAD_Q = 0x51;
// a size query and one call into buffers of exactly the reported sizes (each ends where its allocation ends), against the model; outputs: a subset of "bqlnog"
static int check(rfq_ctx* ctx, const char* what, const Rows& r, const Call& c, size_t shift, uint32_t extra, const char* outputs, int* calls) {
    const Want w = model(r, c);
    const uint32_t T = c.n_bins + (uint32_t)c.rest;
    std::string blob; std::vector<uint64_t> noff; names_of(r, &blob, &noff);
    DevRows d(ctx, r, c, shift, blob, noff);
    rfq_group_rows_args a = d.args(r, c);
    rfq_group_rows_result q, g;
    if (rfq_group_rows(ctx, &d.in, &a, &q)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&q, &w.r, sizeof q)) return fail(what, "the size query's result differs from the host's");
    const uint64_t n = w.r.n_rows; const uint32_t L = extra == 16 ? (w.r.max_len / 16 + 1) * 16 : std::max(w.r.max_len, 1u) + extra;     // (extra 16: the next multiple of 16)
    auto has = [&](char o) { return strchr(outputs, o) != nullptr && (r.named || (o != 'n' && o != 'o')); };
    Dev ob(ctx, nullptr, n * L, shift), oq(ctx, nullptr, n * L, shift), ol(ctx, nullptr, n * 4), on(ctx, nullptr, w.blob.size(), shift), oo(ctx, nullptr, (n + 1) * 8), og(ctx, nullptr, (T + 1) * 8ull);
    a.row_len = L; a.pad_base = PAD_B; a.pad_qual = PAD_Q;
    if (has('b')) { a.d_bases = ob.p; a.bases_cap = n * L; }
    if (has('q')) { a.d_quals = oq.p; a.quals_cap = n * L; }
    if (has('l')) { a.d_lens = (int32_t*)ol.p; a.lens_cap = n; }
    if (has('n')) { a.d_names = on.p; a.names_cap = w.blob.size(); }
    if (has('o')) { a.d_name_off = (uint64_t*)oo.p; a.off_cap = n + 1; }
    if (has('g')) { a.d_bin_off = (uint64_t*)og.p; a.bin_cap = T + 1; }
    if (rfq_group_rows(ctx, &d.in, &a, &g)) return fail(what, rfq_last_error(ctx));
    if (memcmp(&g, &w.r, sizeof g)) return fail(what, "the writing call's result differs from the host's");
    std::vector<uint8_t> hb(n * L + 1), hq(n * L + 1), hn(w.blob.size() + 1); std::vector<int32_t> hl(n + 1); std::vector<uint64_t> ho(n + 2), hg(T + 2);
    if (has('b') && n) rfq_copy_d2h(ctx, hb.data(), ob.p, n * L);
    if (has('q') && n) rfq_copy_d2h(ctx, hq.data(), oq.p, n * L);
    if (has('l') && n) rfq_copy_d2h(ctx, hl.data(), ol.p, n * 4);
    if (has('n') && !w.blob.empty()) rfq_copy_d2h(ctx, hn.data(), on.p, w.blob.size());
    if (has('o')) rfq_copy_d2h(ctx, ho.data(), oo.p, (n + 1) * 8);
    if (has('g')) rfq_copy_d2h(ctx, hg.data(), og.p, (T + 1) * 8ull);
    for (uint64_t j = 0; j < n; j++) {
        const uint32_t src = w.idx[j], s0 = r.start.empty() ? 0 : (uint32_t)r.start[src], wl = (uint32_t)w.lens[j];
        for (uint32_t k = 0; k < L; k++) {
            if (has('b') && hb[j * L + k] != (k < wl ? r.B[(size_t)src * r.L + s0 + k] : PAD_B)) return fail(what, "a base row differs");
            if (has('q') && hq[j * L + k] != (k < wl ? r.Q[(size_t)src * r.L + s0 + k] : PAD_Q)) return fail(what, "a quality row differs");
        }
        if (has('l') && hl[j] != w.lens[j]) return fail(what, "lens differ");
    }
    if (has('n') && memcmp(hn.data(), w.blob.data(), w.blob.size())) return fail(what, "the name blob differs");
    if (has('o') && memcmp(ho.data(), w.name_off.data(), (n + 1) * 8)) return fail(what, "the name offsets differ");
    if (has('g') && memcmp(hg.data(), w.bin_off.data(), (T + 1) * 8ull)) return fail(what, "the bin offsets differ");
    ++*calls;
    return 0;
}
static Call bins_of(uint32_t units, uint32_t n_bins, int rest, int pairs, int pattern) {
    Call c; c.n_bins = n_bins; c.rest = rest; c.pairs = pairs; c.bins.resize(units);
    for (uint32_t u = 0; u < units; u++) {
        int32_t b;
        switch (pattern) {
            case 0: b = (int32_t)(rnd() % (n_bins + 1)) - 1; break;                       // seeded, some negative
            case 1: b = (int32_t)(n_bins / 2); break;                                     // all in one bin
            case 2: b = (int32_t)(u % n_bins); break;                                     // round-robin (a bin of its own where n_bins >= units)
            case 3: b = (int32_t)((units - 1 - u) % n_bins); break;                       // descending
            case 4: b = (int32_t)(((uint64_t)u * n_bins) / units); break;                 // sorted
            case 5: b = (int32_t)((u % 3) << 8); break;                                   // keys that differ in the high byte only
            default: b = (int32_t)(0x300 + u % 7); break;                                 // ... in the low byte only
        }
        c.bins[u] = b;
    }
    if (units > 8) { c.bins[7] = -1; c.bins[8] = INT32_MIN; }
    return c;
}
static int good(rfq_ctx* ctx) {
    int calls = 0;
    const Rows r = make_rows(70, 12, true, true, true);
    return check(ctx, "a good call after a refusal", r, bins_of(35, 3, 1, 1, 0), 0, 0, "bqlnog", &calls);
}
static int refused(rfq_ctx* ctx, const char* what, const rfq_rows_in& in, const rfq_group_rows_args& a, int code, const char* needle) {
    rfq_group_rows_result g;
    const int rc = rfq_group_rows(ctx, &in, &a, &g);
    if (rc != code || !strstr(rfq_last_error(ctx), needle)) { fprintf(stderr, "%s: rc %d, \"%s\" (wanted %d, \"%s\")\n", what, rc, rfq_last_error(ctx), code, needle); return 1; }
    return good(ctx);
}

static const size_t SHIFTS[4] = { 0, 1, 5, 15 };
static const uint32_t GR_TILE = 2048;

int main() {
    rfq_ctx* ctx = nullptr;
    if (rfq_create(&ctx, 0)) { fprintf(stderr, "rfq_create failed\n"); return 1; }
    int bad = 0, calls = 0, refusals = 0;
    // unit counts around a wave, a step and a tile, rows and pairs
    for (uint32_t U : { 0u, 1u, 63u, 64u, 65u, 255u, 256u, 257u, GR_TILE - 1, GR_TILE, GR_TILE + 1, 2 * GR_TILE + 1 }) for (int pairs = 0; pairs < 2 && !bad; pairs++) {
        const Rows r = make_rows(U * (pairs + 1), 9, U % 2 == 1, true, U % 3 == 0);
        bad |= check(ctx, "unit counts", r, bins_of(U, 3, 1, pairs, 0), SHIFTS[U % 4], U % 2 ? 7 : 0, "bqlnog", &calls);
    }
    // totals on both sides of the seam and at the limits, the rest bin kept and dropped
    for (uint32_t T : { 1u, 2u, 255u, 256u, 257u, 4097u, 65536u }) for (int rest = 0; rest < 2 && !bad; rest++) {
        if (T - (uint32_t)rest < 1) continue;
        const Rows r = make_rows(300, 12, true, false, false);
        bad |= check(ctx, "totals", r, bins_of(300, T - (uint32_t)rest, rest, 0, 0), 0, 0, "bqlnog", &calls);
    }
    // the patterns over one pass and two
    for (int pattern = 1; pattern <= 6 && !bad; pattern++) for (uint32_t n_bins : { 256u, 1024u }) {
        if (pattern >= 5 && n_bins == 256) continue;
        const Rows r = make_rows(200, 10, true, false, true);
        bad |= check(ctx, "patterns", r, bins_of(200, n_bins, (int)(n_bins == 1024), 0, pattern), 5, 0, "bqlnog", &calls);
    }
    if (!bad) {   // layout: unaligned with strides that are no multiple of 16, aligned with multiples; min_len; rows without names; nothing kept; many units
        Rows r = make_rows(120, 37, true, true, true);
        bad |= check(ctx, "unaligned", r, bins_of(120, 4, 1, 0, 0), 5, 1, "bqlnog", &calls);
        r = make_rows(120, 48, true, true, true);
        Call c = bins_of(60, 4, 0, 1, 0); c.min_len = 20;
        bad |= check(ctx, "aligned, pairs, min_len 20", r, c, 0, 16, "bqlnog", &calls);
        r = make_rows(150, 7, false, true, false);
        bad |= check(ctx, "rows without names", r, bins_of(150, 5, 1, 0, 0), 1, 0, "bqlg", &calls);
        r = make_rows(66, 8, true, false, false); r.keep.assign(66, 0);
        bad |= check(ctx, "nothing kept", r, bins_of(66, 3, 1, 0, 2), 0, 0, "bqlnog", &calls);
        r = make_rows(40003, 4, true, true, false);
        bad |= check(ctx, "40003 units", r, bins_of(40003, 300, 1, 0, 0), 1, 0, "bqlnog", &calls);
        r = make_rows(300, 20, true, true, false);
        for (const char* o : { "g", "l", "bqlg", "no", "b", "n" }) bad |= check(ctx, "partial outputs", r, bins_of(300, 10, 1, 0, 0), 0, 0, o, &calls);
    }
    if (!bad) {   // the refusals
        const Rows r = make_rows(40, 16, true, true, true);
        const Call c = bins_of(40, 3, 1, 0, 2);
        std::string blob; std::vector<uint64_t> noff; names_of(r, &blob, &noff);
        DevRows d(ctx, r, c, 0, blob, noff);
        Dev out(ctx, nullptr, 65536);
        const rfq_rows_in in = d.in;
        const rfq_group_rows_args a0 = d.args(r, c);
        rfq_group_rows_args a; rfq_rows_in x;
        auto with_rows = [&](rfq_group_rows_args& t) { t.row_len = 16; t.d_bases = out.p; t.bases_cap = 640; };
#define REFUSED(what, X, A, needle) do { bad |= refused(ctx, what, X, A, RFQ_E_ARG, needle); refusals++; } while (0)
        a = a0; a.pairs = 1; x = in; x.n_rows = 39; REFUSED("an odd row count", x, a, "rows in pairs");
        a = a0; a.pairs = 2; REFUSED("pairs 2", in, a, "0 or 1");
        a = a0; with_rows(a); a.row_len = 0; REFUSED("row_len 0", in, a, "row_len must be >= 1");
        x = in; x.row_len = 0; REFUSED("the rows' row_len 0", x, a0, "row_len");
        x = in; x.n_rows = 0xFFFFFFF0ull; REFUSED("2^32 - 16 rows", x, a0, "too many");
        a = a0; a.d_bin = nullptr; REFUSED("null d_bin", in, a, "null d_bin");
        x = in; x.d_lens = nullptr; REFUSED("null d_lens", x, a0, "null");
        a = a0; a.n_bins = 0; REFUSED("n_bins 0", in, a, "n_bins must be >= 1");
        a = a0; a.n_bins = 65536; REFUSED("T 65537", in, a, "at most 65536");
        a = a0; a.n_bins = 0xFFFFFFFFu; REFUSED("T 2^32", in, a, "at most 65536");
        a = a0; a.rest = 2; REFUSED("rest 2", in, a, "rest must be 0 or 1");
        a = a0; a.rest = -1; REFUSED("rest -1", in, a, "rest must be 0 or 1");
        a = a0; a.d_bin = (const int32_t*)(d.bin.p + 2); REFUSED("misaligned d_bin", in, a, "4-byte");
        a = a0; a.d_start = (const int32_t*)(d.start.p + 1); REFUSED("misaligned d_start", in, a, "4-byte");
        a = a0; with_rows(a); a.d_lens = (int32_t*)(out.p + 1026); a.lens_cap = 40; REFUSED("misaligned out d_lens", in, a, "4-byte");
        x = in; x.d_name_off = (const uint64_t*)(d.off.p + 4); REFUSED("misaligned in d_name_off", x, a0, "8-byte");
        a = a0; a.d_bin_off = (uint64_t*)(out.p + 4); a.bin_cap = 5; REFUSED("misaligned d_bin_off", in, a, "d_bin_off must be 8-byte aligned");
        a = a0; with_rows(a); a.d_bases = d.b.p; REFUSED("bases on bases", in, a, "overlaps the input rows->d_bases");
        a = a0; with_rows(a); a.d_bases = nullptr; a.d_lens = (int32_t*)d.bin.p; a.lens_cap = 40; REFUSED("lens on d_bin", in, a, "d_lens overlaps the input d_bin");
        a = a0; a.d_bin_off = (uint64_t*)(d.bin.p + 8 - (uintptr_t)d.bin.p % 8); a.bin_cap = 5; REFUSED("bin_off on d_bin", in, a, "d_bin_off overlaps the input d_bin");
        a = a0; a.d_bin_off = (uint64_t*)(d.l.p + 8 - (uintptr_t)d.l.p % 8); a.bin_cap = 5; REFUSED("bin_off on lens", in, a, "d_bin_off overlaps the input rows->d_lens");
        { Rows r2 = r; r2.named = false; DevRows d2(ctx, r2, c, 0, "", {}); a = d2.args(r2, c); with_rows(a); a.d_bases = nullptr; a.d_name_off = (uint64_t*)out.p; a.off_cap = 41;
          REFUSED("name outputs for rows without names", d2.in, a, "rows without names"); }
        // RFQ_E_NOSPACE: every cap one short
        { const Want w = model(r, c); const uint64_t n = w.r.n_rows; const uint32_t L = w.r.max_len;
          for (int k = 0; k < 7 && !bad; k++) {
              a = a0; a.row_len = L; a.d_bases = out.p; a.bases_cap = n * L; a.d_quals = out.p + 8192; a.quals_cap = n * L; a.d_lens = (int32_t*)(out.p + 16384); a.lens_cap = n;
              a.d_names = out.p + 24576; a.names_cap = w.blob.size(); a.d_name_off = (uint64_t*)(out.p + 32768); a.off_cap = n + 1; a.d_bin_off = (uint64_t*)(out.p + 40960); a.bin_cap = 5;
              switch (k) { case 0: a.row_len--; break; case 1: a.bases_cap--; break; case 2: a.quals_cap--; break; case 3: a.lens_cap--; break; case 4: a.names_cap--; break;
                           case 5: a.off_cap--; break; default: a.bin_cap--; break; }
              bad |= refused(ctx, "a cap one short", in, a, RFQ_E_NOSPACE, k == 6 ? "bin_cap < T + 1" : "need"); refusals++;
          } }
        // on the device: bin == n_bins and INT32_MAX in the first unit, the last and a masked one, rows and pairs, alone and beside a bad length and a bad window
        for (int32_t v : { 3, INT32_MAX }) for (uint32_t unit : { 0u, 19u, 9u }) for (int pairs = 0; pairs < 2; pairs++) for (int beside = 0; beside < 3 && !bad; beside++) {
            Rows r2 = r; Call c2 = bins_of(pairs ? 20 : 40, 3, 1, pairs, 2);
            const uint32_t u = pairs ? unit : 2 * unit + (unit ? 1 : 0), nr = pairs ? 2 : 1;
            c2.bins[u] = v;
            if (unit == 9u) for (uint32_t i = 0; i < nr; i++) r2.keep[nr * u + i] = 0;
            if (beside == 1) r2.lens[30] = 17;
            if (beside == 2) r2.start[31] = -1;
            DevRows d2(ctx, r2, c2, 1, blob, noff);
            a = d2.args(r2, c2); with_rows(a); a.d_bin_off = (uint64_t*)(out.p + 4096); a.bin_cap = 5;
            char needle[64]; snprintf(needle, sizeof needle, beside == 0 ? "first such unit: %u)" : "first such row: %u)", beside == 0 ? u : 29u + (uint32_t)beside);
            REFUSED("a bad bin", d2.in, a, needle);
        }
#undef REFUSED
    }
    rfq_destroy(ctx);
    if (bad) return 1;
    printf("group_asan: %d good calls (units 0 .. 2 tiles + 1 and 40003, totals 1 .. 65536 on both sides of the one-pass / two-pass seam, the bin patterns, the rest bin kept and "
           "dropped, rows and pairs, masks, windows, min_len, with and without names, shifts 0 / 1 / 5 / 15, partial outputs) and %d refusals (host, RFQ_E_NOSPACE and device) each "
           "followed by a good call: all as the host loop says, no sanitizer report\n", calls, refusals);
    return 0;
}
