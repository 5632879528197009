// tests/ranges_main.cpp — the decode path's range plan (repaq_amd/csrc/dec/ranges.h) over synthetic chunk tables: test_ranges.py compiles this with
// g++ and runs it; no library, no GPU.  The header comes after <vector> and <cstdint> alone: it has to stand on those.
#include <vector>
#include <cstdint>
#include "dec/ranges.h"
#include <cstdio>
#include <string>

struct Chunk { uint64_t off; uint32_t reads, flags; uint64_t bases; };      // the fields of DChunk the header reads
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t sum_bases(const std::vector<Chunk>& hc, const ChunkSpan& r) { uint64_t s = 0; for (uint32_t c = r.c0; c < r.c1; c++) s += hc[c].bases; return s; }
static uint64_t sum_reads(const std::vector<Chunk>& hc, const ChunkSpan& r) { uint64_t s = 0; for (uint32_t c = r.c0; c < r.c1; c++) s += hc[c].reads; return s; }

// the loop of dec_each_range (rfq_decode.hip) with a body that calls every span of more than k chunks too big.  false: a single chunk was too big.
// steps: a walk that went round more often than halving n chunks down to single ones can take is looping
static bool walk(RangeQueue q, const std::vector<Chunk>& hc, uint32_t k, std::vector<ChunkSpan>* accepted, bool* looped) {
    size_t steps = 0; const size_t most = 4 * hc.size() + 16; *looped = false;
    for (ChunkSpan r; q.next(&r);) {
        if (++steps > most) { *looped = true; return false; }
        if (sum_reads(hc, r) >= RANGE_MAX_READS || r.c1 - r.c0 > k) { if (!q.halve(r)) return false; continue; }
        accepted->push_back(r);
    }
    return true;
}
// spans tile the pieces in order: no gap, no overlap, none across a piece's end, r1_only the piece's
static void check_tiling(const char* what, const std::vector<ChunkSpan>& spans, const std::vector<ChunkSpan>& pieces, uint32_t most_chunks) {
    size_t i = 0;
    for (auto& pc : pieces) {
        uint32_t at = pc.c0;
        while (at < pc.c1) {
            CHECK(i < spans.size(), "%s: spans end at chunk %u of piece [%u, %u)", what, at, pc.c0, pc.c1);
            if (i >= spans.size()) return;
            const ChunkSpan& r = spans[i++];
            CHECK(r.c0 == at && r.c1 > r.c0 && r.c1 <= pc.c1 && r.r1_only == pc.r1_only, "%s: span [%u, %u) r1_only %d at chunk %u of piece [%u, %u) r1_only %d", what, r.c0, r.c1,
                  (int)r.r1_only, at, pc.c0, pc.c1, (int)pc.r1_only);
            CHECK(r.c1 - r.c0 <= most_chunks, "%s: span [%u, %u) has more than %u chunks", what, r.c0, r.c1, most_chunks);
            if (r.c1 <= at) return;
            at = r.c1;
        }
    }
    CHECK(i == spans.size(), "%s: %zu spans behind the last piece", what, spans.size() - i);
}

struct Table { std::string name; std::vector<Chunk> hc; uint64_t slice_bases; };
static std::vector<Table> tables(uint32_t n) {
    std::vector<Table> t; const std::string sn = std::to_string(n);
    auto make = [&](const char* name, uint64_t slice, auto fill) { Table x; x.name = name + ("/" + sn); x.slice_bases = slice; x.hc.resize(n);
        for (uint32_t c = 0; c < n; c++) { x.hc[c].off = 100 + 10ull * c; x.hc[c].flags = 0; fill(c, x.hc[c]); } t.push_back(x); };
    make("even", 45000, [](uint32_t, Chunk& h) { h.reads = 134; h.bases = 20000; });                            // (the shape of the forced-ranges tests: two chunks per range)
    make("uneven", 45000, [](uint32_t c, Chunk& h) { h.reads = 1 + c * 37 % 200; h.bases = 150ull * h.reads; });
    make("exact_fit", 40000, [](uint32_t, Chunk& h) { h.reads = 100; h.bases = 20000; });                       // (two chunks are exactly slice_bases: not cut)
    make("first_chunk_above_slice", 45000, [](uint32_t c, Chunk& h) { h.reads = 134; h.bases = c ? 20000 : 50000; });
    make("every_chunk_above_slice", 1000, [](uint32_t, Chunk& h) { h.reads = 134; h.bases = 20000; });
    make("zero_reads", 45000, [](uint32_t c, Chunk& h) { h.reads = c % 3 == 1 ? 134 : 0; h.bases = 150ull * h.reads; });
    make("all_zero_reads", 45000, [](uint32_t, Chunk& h) { h.reads = 0; h.bases = 0; });
    // counts only: the read sum crosses RANGE_MAX_READS inside the table while the bases stay far below the slice
    make("reads_cross_the_limit", 1500000000ull, [](uint32_t, Chunk& h) { h.reads = 0x30000000u; h.bases = 1000; });
    make("reads_reach_the_limit_exactly", 1500000000ull, [](uint32_t c, Chunk& h) { h.reads = c % 2 ? 0x3FFFFFF0u : 0x40000000u; h.bases = 1000; });
    make("default_slice", 1500000000ull, [](uint32_t c, Chunk& h) { h.reads = 4000000; h.bases = 600000000ull + c; });
    return t;
}
// one piece, and the image in several: a run, one chunk of which only R1 is written, the rest (bug_compat's shape)
static std::vector<std::vector<ChunkSpan>> piece_lists(uint32_t n) {
    std::vector<std::vector<ChunkSpan>> p; p.push_back({ { 0, n, false } });
    if (n >= 2) p.push_back({ { 0, 1, true }, { 1, n, false } });
    if (n >= 3) { p.push_back({ { 0, n / 2, false }, { n / 2, n / 2 + 1, true }, { n / 2 + 1, n, false } }); p.push_back({ { 0, n - 1, true }, { n - 1, n, false } }); }
    return p;
}

static void check_plan() {
    for (uint32_t n : { 1u, 2u, 3u, 7u, 64u }) for (auto& t : tables(n)) for (auto& pieces : piece_lists(n)) {
        const char* nm = t.name.c_str();
        const RangeQueue q = plan_ranges(pieces, t.hc.data(), t.slice_bases);
        // ---- tiling and limits of the plan itself
        std::vector<ChunkSpan> planned; { RangeQueue w = q; for (ChunkSpan r; w.next(&r);) planned.push_back(r); }
        check_tiling(nm, planned, pieces, n);
        for (auto& r : planned) if (r.c1 - r.c0 >= 2) {
            CHECK(sum_bases(t.hc, r) <= t.slice_bases, "%s: span [%u, %u) holds %llu bases", nm, r.c0, r.c1, (unsigned long long)sum_bases(t.hc, r));
            CHECK(sum_reads(t.hc, r) < RANGE_MAX_READS, "%s: span [%u, %u) holds %llu reads", nm, r.c0, r.c1, (unsigned long long)sum_reads(t.hc, r));
        }
        // (the plan does not cut more often than the limits ask for: two neighbours of one piece never fit one span)
        for (size_t i = 0; i + 1 < planned.size(); i++) {
            const ChunkSpan &x = planned[i], &y = planned[i + 1]; bool same = false;
            for (auto& pc : pieces) same |= x.c0 >= pc.c0 && y.c1 <= pc.c1;
            if (same) CHECK(sum_bases(t.hc, x) + t.hc[y.c0].bases > t.slice_bases || sum_reads(t.hc, x) + t.hc[y.c0].reads >= RANGE_MAX_READS, "%s: cut at chunk %u for nothing", nm, y.c0);
        }
        // ---- halving: the accepted spans still tile the pieces, none of more than k chunks; a single chunk that is too big ends the walk
        bool single_too_big = false; for (auto& h : t.hc) single_too_big |= h.reads >= RANGE_MAX_READS;
        for (uint32_t k : { 1u, 2u, 5u }) {
            std::vector<ChunkSpan> acc; bool looped = false;
            const bool ok = walk(q, t.hc, k, &acc, &looped);
            CHECK(!looped, "%s k=%u: the walk does not end", nm, k);
            CHECK(ok == !single_too_big, "%s k=%u: walk %s", nm, k, ok ? "passed" : "failed");
            if (ok) check_tiling(nm, acc, pieces, k);
        }
        { std::vector<ChunkSpan> acc; bool looped = false;                      // k = 0: every single chunk is too big - failure at the first, no loop
          CHECK(!walk(q, t.hc, 0, &acc, &looped) && !looped && acc.empty(), "%s k=0: a chunk that cannot be halved must end the walk", nm); }
    }
    // a single chunk beyond the read limit: planned as a span of its own, refused without looping, whatever stands around it
    for (uint32_t at : { 0u, 3u, 6u }) {
        std::vector<Chunk> hc(7); for (auto& h : hc) { h.reads = 100; h.bases = 15000; } hc[at].reads = 0x7FFFFFF0u;
        const RangeQueue q = plan_ranges(std::vector<ChunkSpan>{ { 0, 7, false } }, hc.data(), 1500000000ull);
        std::vector<ChunkSpan> acc; bool looped = false;
        CHECK(!walk(q, hc, 5, &acc, &looped) && !looped, "big chunk at %u: the walk must fail", at);
        for (auto& r : acc) CHECK(r.c1 <= at, "big chunk at %u: span [%u, %u) accepted behind it", at, r.c0, r.c1);
    }
    // halve: front half next, back half behind it, the r1_only mark on both
    { RangeQueue q; q.todo.push_back({ 9, 10, false }); ChunkSpan a = { 0, 0, false }, b = a, c = a;
      CHECK(q.halve({ 2, 7, true }) && q.next(&a) && q.next(&b) && q.next(&c) && !q.next(&c), "halve");
      CHECK(a.c0 == 2 && a.c1 == 4 && a.r1_only && b.c0 == 4 && b.c1 == 7 && b.r1_only && c.c0 == 9, "halve: [%u, %u) [%u, %u) [%u, %u)", a.c0, a.c1, b.c0, b.c1, c.c0, c.c1);
      CHECK(!q.halve({ 5, 6, false }) && !q.next(&a), "a single chunk must not be halved"); }
}

// compat_pieces against the table of the code it was taken out of (rfq_decode_batch before the range plan became a header: recorded from that loop,
// not from this one).  flags per chunk: 1 = the R1 NO_LINE_BREAK bit, 2 = R2's; chunk i starts at byte 100 + 10 i, the walk consumed 100 + 10 n;
// pieces as "c0-c1 ", "c0-c1r " where only R1 is written.  The patterns are those of tests/golden/compat.json's cases: flagged first, flagged last
// with and without final, two flagged in a row, the R1 bit against the R2 bit with split, one output.
struct CompatCase { const char* name; std::vector<int> flags; int split, final; const char* pieces; int strip1, strip2; uint32_t n_chunks; uint64_t consumed; };
static void check_compat() {
    const uint32_t B1 = 1u << 10, B2 = 1u << 11;
    const std::vector<CompatCase> cases = {
        { "none", { 0, 0, 0 }, 1, 1, "0-3 ", 0, 0, 3, 130 },
        { "first_r1", { 1, 0, 0, 0 }, 1, 1, "0-1r 2-4 ", 0, 0, 3, 140 },
        { "first_r2", { 2, 0, 0, 0 }, 1, 1, "0-1 2-4 ", 0, 0, 3, 140 },
        { "first_both", { 3, 0, 0, 0 }, 1, 1, "0-1r 2-4 ", 0, 0, 3, 140 },
        { "middle_r1", { 0, 0, 1, 0, 0 }, 1, 1, "0-2 2-3r 4-5 ", 0, 0, 4, 150 },
        { "middle_r2", { 0, 0, 2, 0, 0 }, 1, 1, "0-3 4-5 ", 0, 0, 4, 150 },
        { "middle_r1_one_output", { 0, 0, 1, 0, 0 }, 0, 1, "0-3 4-5 ", 0, 0, 4, 150 },
        { "middle_r2_one_output", { 0, 0, 2, 0, 0 }, 0, 1, "0-5 ", 0, 0, 5, 150 },
        { "last_r1_final", { 0, 0, 1 }, 1, 1, "0-3 ", 1, 0, 3, 130 },
        { "last_r2_final", { 0, 0, 2 }, 1, 1, "0-3 ", 0, 1, 3, 130 },
        { "last_both_final", { 0, 0, 3 }, 1, 1, "0-3 ", 1, 1, 3, 130 },
        { "last_r1_not_final", { 0, 0, 1 }, 1, 0, "0-2 ", 0, 0, 2, 120 },
        { "last_r2_not_final", { 0, 0, 2 }, 1, 0, "0-2 ", 0, 0, 2, 120 },
        { "only_chunk_final", { 1 }, 1, 1, "0-1 ", 1, 0, 1, 110 },
        { "only_chunk_not_final", { 1 }, 1, 0, "", 0, 0, 0, 100 },
        { "two_in_a_row", { 0, 1, 1, 0, 0 }, 1, 1, "0-1 1-2r 3-5 ", 0, 0, 4, 150 },
        { "two_in_a_row_r2", { 0, 2, 2, 0, 0 }, 1, 1, "0-2 3-5 ", 0, 0, 4, 150 },
        { "two_in_a_row_at_the_end", { 0, 1, 1 }, 1, 1, "0-1 1-2r ", 0, 0, 2, 130 },
        { "three_in_a_row", { 1, 1, 1, 0 }, 1, 1, "0-1r 2-3r ", 0, 0, 2, 140 },
        { "every_third", { 0, 0, 3, 0, 0, 3, 0, 0, 3, 0 }, 1, 1, "0-2 2-3r 4-5 5-6r 7-8 8-9r ", 0, 0, 7, 200 },
        { "flagged_then_last_flagged_not_final", { 0, 1, 0, 2 }, 1, 0, "0-1 1-2r ", 0, 0, 2, 130 },
        { "second_to_last_r1_final", { 0, 0, 1, 0 }, 1, 1, "0-2 2-3r ", 0, 0, 3, 140 },
    };
    for (auto& cs : cases) {
        const uint32_t n = (uint32_t)cs.flags.size(); std::vector<Chunk> hc(n);
        for (uint32_t i = 0; i < n; i++) { hc[i].off = 100 + 10ull * i; hc[i].reads = 134; hc[i].bases = 20000; hc[i].flags = (cs.flags[i] & 1 ? B1 : 0) | (cs.flags[i] & 2 ? B2 : 0) | 5u; }
        const CompatPlan p = compat_pieces(hc.data(), n, cs.split != 0, cs.final != 0, 100 + 10ull * n, B1, B2);
        std::string s; for (auto& q : p.pieces) s += std::to_string(q.c0) + "-" + std::to_string(q.c1) + (q.r1_only ? "r " : " ");
        CHECK(s == cs.pieces, "%s: pieces \"%s\", want \"%s\"", cs.name, s.c_str(), cs.pieces);
        CHECK((int)p.strip1 == cs.strip1 && (int)p.strip2 == cs.strip2, "%s: strip %d %d", cs.name, (int)p.strip1, (int)p.strip2);
        CHECK(p.n_chunks == cs.n_chunks && p.consumed == cs.consumed, "%s: %u chunks, consumed %llu", cs.name, p.n_chunks, (unsigned long long)p.consumed);
        // and the pieces through the plan: ranges of two chunks, the R1-only mark carried through
        std::vector<ChunkSpan> planned; { RangeQueue w = plan_ranges(p.pieces, hc.data(), 45000); for (ChunkSpan r; w.next(&r);) planned.push_back(r); }
        check_tiling(cs.name, planned, p.pieces, 2);
    }
}

int main() {
    check_plan();
    check_compat();
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("RANGES_OK\n");
    return 0;
}
