// dec/ranges.h — which chunks of an image one decode pass takes.  Host code only (no HIP: tests/ranges_main.cpp drives it under plain g++).
// Reads, bases and text of one pass are placed by 32-bit prefix sums: a larger image is decoded range by range - contiguous chunks cut out of every
// piece [c0, c1) of the image.  The chunk table is anything with .reads and .bases per chunk (DChunk, dec/chunk_walk.h; compat_pieces: .flags and .off too).
#pragma once
#include <cstdint>
#include <vector>

#define RANGE_MAX_READS 0x7FFFFFF0ull     // a pass counts its reads in 32 bits (+ 2 entries of slack, signed offsets in the kernels)
#define RANGE_MAX_BASES 0xFFFFFFF0ull     // and its bases

// the chunks [c0, c1) of the image (r1_only: a piece of which the reference writes the first mate only)
struct ChunkSpan { uint32_t c0, c1; bool r1_only; };

// the spans still to decode, handed out in image order
struct RangeQueue {
    std::vector<ChunkSpan> todo;                                              // a stack: the next span on top
    bool next(ChunkSpan* r) { if (todo.empty()) return false; *r = todo.back(); todo.pop_back(); return true; }
    // a span that turned out too big for one pass: its front half comes next, its back half after that.  false: a single chunk cannot be halved
    bool halve(const ChunkSpan& r) {
        const uint32_t mid = r.c0 + (r.c1 - r.c0) / 2;
        if (mid == r.c0) return false;
        todo.push_back({ mid, r.c1, r.r1_only }); todo.push_back({ r.c0, mid, r.r1_only }); return true;
    }
};
// The cut rule: a span ends in front of the chunk that would take it past slice_bases bases or up to RANGE_MAX_READS reads, so a span of two or
// more chunks stays within both; a single chunk may exceed them (nothing to cut: the decode refuses it).  Spans never cross a piece.
template <class Chunk>
static RangeQueue plan_ranges(const std::vector<ChunkSpan>& pieces, const Chunk* hc, uint64_t slice_bases) {
    std::vector<ChunkSpan> fw; RangeQueue q;
    for (auto& pc : pieces) {
        uint32_t c0 = pc.c0; uint64_t acc = 0, rd = 0;
        for (uint32_t c = pc.c0; c < pc.c1; c++) {
            if (c > c0 && (acc + hc[c].bases > slice_bases || rd + hc[c].reads >= RANGE_MAX_READS)) { fw.push_back({ c0, c, pc.r1_only }); c0 = c; acc = 0; rd = 0; }
            acc += hc[c].bases; rd += hc[c].reads;
        }
        fw.push_back({ c0, pc.c1, pc.r1_only });
    }
    q.todo.assign(fw.rbegin(), fw.rend());
    return q;
}

// bug_compat: Repaq::decompressPE as it stands (src/repaq.cpp:330-417).  A chunk with a NO_LINE_BREAK bit makes the loop read the chunk behind it
// to see whether it was the last (:376-387); when it was not, `continue` (:389-392, :400-403) goes on with a fresh read - decompressPE declares
// its chunk inside the loop - and the chunk it peeked at is never decoded; it also leaves the body before the flagged chunk's R2 text is written
// when it is the R1 bit that is set.  The text is decoded piece by piece: runs of chunks that survive, R1 only where the reference drops R2.
// Repaq::decompress (one output, :262-328) peeks the same way but keeps the peeked chunk in a variable that outlives the iteration and decodes it
// next: nothing is lost there, and the only effect of the bit - the last chunk's final '\n' dropped - is the default behaviour.
// nolb1 / nolb2: the NO_LINE_BREAK bits of R1 / R2 in a chunk's flags.  consumed: the walk's, moved back in front of a flagged last chunk of a
// slice that does not end the image (the caller has to show what follows: the chunk stays unconsumed).
struct CompatPlan { std::vector<ChunkSpan> pieces; bool strip1 = false, strip2 = false; uint32_t n_chunks = 0; uint64_t consumed = 0; };
template <class Chunk>
static CompatPlan compat_pieces(const Chunk* hc, uint32_t n_chunks, bool split, bool final, uint64_t consumed, uint32_t nolb1, uint32_t nolb2) {
    CompatPlan p; p.consumed = consumed;
    uint32_t run = 0, end = n_chunks;
    for (uint32_t i = 0; i < n_chunks;) {
        const bool f1 = (hc[i].flags & nolb1) != 0, f2 = split && (hc[i].flags & nolb2) != 0;
        if (!f1 && !f2) { i++; continue; }
        if (i + 1 == n_chunks) {                                            // nothing behind it in this image
            if (!final) { end = i; p.consumed = hc[i].off; }
            else { p.strip1 = f1; p.strip2 = f2; }
            break;
        }
        if (split && f1) { if (i > run) p.pieces.push_back({ run, i, false }); p.pieces.push_back({ i, i + 1, true }); }
        else p.pieces.push_back({ run, i + 1, false });
        run = i + 2; i += 2;                                                // (the chunk behind a flagged one that is not the last: lost)
    }
    if (run < end) p.pieces.push_back({ run, end, false });
    for (auto& q : p.pieces) p.n_chunks += q.c1 - q.c0;
    return p;
}
