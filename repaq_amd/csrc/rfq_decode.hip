// rfq_decode.hip — host orchestration of the gfx950 RFQ -> FASTQ path (rfq_decode_batch of include/rfq_hip.h).
// Replaces, per image: RfqHeader::read (src/rfqheader.cpp:19-43), RfqChunk::read (src/rfqchunk.cpp:161-228),
// RfqCodec::decodeChunk (src/rfqcodec.cpp:826-1260) and the text emission of Repaq::decompress / decompressPE
// (src/repaq.cpp:262-417; final-newline rule :301-328,375-413).
#include "rfq_ctx.h"
#include "rfq_decode_kernels.h"
#include "dec/ranges.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>

int rfq_upload_header(rfq_ctx* c, const uint8_t* h, size_t n);   // rfq_encode.hip

enum DecBuf {   // indices into rfq_ctx::b (disjoint from the encoder's, so one context can alternate encode / decode)
    DB_CHUNKS = 80, DB_STATUS, DB_LEN, DB_CHUNKID, DB_OV, DB_PVIN, DB_PV, DB_PQ, DB_TIN, DB_TP, DB_QBASE, DB_SBASE, DB_QDEC, DB_SDEC, DB_XV, DB_YV, DB_SCAN, DB_MID, DB_SEGF, DB_SEGA, DB_SEGN, DB_SEGS, DB_SEGP, DB_OFFT, DB_CELL, DB_SEGK, DB_NENT, DB_LOFF, DB_PLIST, DB_GWCAND, DB_GWLIST, DB_GWCNT, DB_GWLAND, DB_PQL, DB_PVL, DB_TPL, DB_CTEXT, DB_TBASE, DB_SDL, DB_END
};
static_assert(DB_END <= 120, "rfq_ctx::b too small");

#define RFQ_RANGE_TOO_BIG 2          // internal: the range's text would not fit the 32-bit text offsets of one pass
// bases: sum of the range's read lengths (the walk's 64-bit total)
struct DecRange { const DChunk* CH; uint32_t n_chunks, n_reads, max_reads, max_stream, max_npos, max_len, max_bases, max_nrec, max_one, per_read_pieces, piece_avg, piece_n1;
        uint64_t bases; };
// the nine maxima of a walk: from the status behind the second parse to the first one's (dec_walk), from the walk's status to a range (range_of)
template <class D, class S> static void take_maxima(D& d, const S& s) {
    d.max_stream = s.max_stream; d.max_npos = s.max_npos; d.max_len = s.max_len; d.max_bases = s.max_bases; d.max_nrec = s.max_nrec;
    d.max_one = s.max_one; d.per_read_pieces = s.per_read_pieces; d.piece_avg = s.piece_avg; d.piece_n1 = s.piece_n1;
}
// ---- the expanded stage of a range (the text path's fallback emitter and rfq_decode_rows read what it leaves in HBM)
// read table: per-read values (k_dec_readtab), the quality / stored-base prefixes (two scans), their totals read back.  text: the text bookkeeping
// (tin / tp, filled by k_dec_textlen) is allocated too.  R.len / R.ov / R.mid are the caller's.
static int dec_table_expanded(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, DReadTab& R, bool text, uint32_t* total_bases, U4* pv_tot) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>(); DecStatus* dst = B[DB_STATUS].as<DecStatus>();
    const uint32_t n_chunks = g.n_chunks, n_reads = g.n_reads, max_reads = std::max(g.max_reads, 1u);
    const size_t nr = (size_t)n_reads + 2, nc = (size_t)n_chunks + 2;
    HIPCHK(ctx, B[DB_CHUNKID].ensure(nr * 4));
    HIPCHK(ctx, B[DB_PVIN].ensure(nr * 16)); HIPCHK(ctx, B[DB_PV].ensure(nr * 16)); HIPCHK(ctx, B[DB_PQ].ensure(nr * 4));
    if (text) { HIPCHK(ctx, B[DB_TIN].ensure(nr * 16)); HIPCHK(ctx, B[DB_TP].ensure(nr * 16)); }
    HIPCHK(ctx, B[DB_QBASE].ensure(nc * 8)); HIPCHK(ctx, B[DB_SBASE].ensure(nc * 8));
    HIPCHK(ctx, B[DB_SCAN].ensure((nr / SCAN_TILE + 2) * 16 + 1024));
    R.chunk = B[DB_CHUNKID].as<uint32_t>();
    R.pvin = B[DB_PVIN].as<U4>(); R.pv = B[DB_PV].as<U4>(); R.pq = B[DB_PQ].as<uint32_t>();
    R.tin = text ? B[DB_TIN].as<U4>() : nullptr; R.tp = text ? B[DB_TP].as<U4>() : nullptr;
    hipLaunchKernelGGL(k_dec_readtab, dim3((max_reads + 255) / 256, n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, D, R, dst);
    KCHK(ctx, "k_dec_readtab");
    scan_exclusive<uint32_t>(S, R.len, R.pq, n_reads, B[DB_SCAN].as<uint32_t>(), 1);
    scan_exclusive<U4>(S, R.pvin, R.pv, n_reads, B[DB_SCAN].as<U4>(), 1);
    HIPCHK(ctx, ctx->fetch(total_bases, R.pq + n_reads, 4, S));
    HIPCHK(ctx, ctx->fetch(pv_tot, R.pv + n_reads, 16, S));
    DecStatus h2; HIPCHK(ctx, ctx->fetch(&h2, dst, sizeof h2, S)); HIPCHK(ctx, ctx->fetch_sync(S));
    ctx->timer.end(S);
    if (h2.err & DE_CORRUPT) return rfq_fail(ctx, RFQ_E_FORMAT, "corrupt overlap buffer");
    return RFQ_OK;
}
// qualities and stored bases expanded into qdec / sdec (k_dec_bases, fill, unpack, position streams, exception records, RLE), timer stage "streams".
// coords: the coordinate decoder rides along on the main stream (the text path's name lines need it; rows do not)
struct DecExpanded { uint64_t* qbase; uint64_t* sbase; uint8_t* qdec; uint8_t* sdec; size_t qbytes, sbytes; };
static int dec_streams_expanded(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const DReadTab& R, uint32_t total_bases, const U4& pv_tot, bool coords,
                                DecExpanded* E) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader& HH = ctx->h_hdr; const DevHeader* D = ctx->d_hdr.as<DevHeader>();
    DecStatus* dst = B[DB_STATUS].as<DecStatus>(); const DChunk* CH = g.CH; const uint32_t n_chunks = g.n_chunks; const size_t nc = (size_t)n_chunks + 2;
    const bool rle_h = !(HH.flags & (H_DONT_QUAL | H_QUAL_BY_COL));
    ctx->timer.begin("streams", S);
    const size_t qbytes = (size_t)total_bases + 64 * nc + 256, sbytes = (size_t)pv_tot.d + 64 * nc + 256;
    HIPCHK(ctx, B[DB_QDEC].ensure(qbytes)); HIPCHK(ctx, B[DB_SDEC].ensure(sbytes));
    uint64_t* const qbase = B[DB_QBASE].as<uint64_t>(); uint64_t* const sbase = B[DB_SBASE].as<uint64_t>();
    uint8_t* const qdec = B[DB_QDEC].as<uint8_t>(); uint8_t* const sdec = B[DB_SDEC].as<uint8_t>();
    hipLaunchKernelGGL(k_dec_bases, dim3((n_chunks + 255) / 256), dim3(256), 0, S, CH, R, qbase, sbase, n_chunks);
    // Two chains run side by side (rfq_ctx::aux, fork / join by events):
    //   main  prefill of qdec, coordinate decoder, [summaries linked] quality position streams scattered into qdec, exception records
    //   aux   position-stream summaries + link, 2-bit unpack into sdec, N positions scattered into sdec
    const bool forked = ctx->aux_ready();
    hipStream_t A = forked ? ctx->aux : S;
    if (forked) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(A, ctx->ev_fork, 0)); }
    const uint32_t bpc = std::max(1u, std::min(64u, 4096u / n_chunks));
    // the prefill is pure bandwidth, the coordinate decoder and the stream summaries are pure latency: third chain
    hipStream_t F = forked ? ctx->aux2 : S;
    if (forked) HIPCHK(ctx, hipStreamWaitEvent(F, ctx->ev_fork, 0));
    // (many short blocks: slots keep turning over for the two other chains)
    hipLaunchKernelGGL(k_dec_fill, dim3((uint32_t)std::min<size_t>(8192, (qbytes / 16 + 255) / 256 + 1)), dim3(256), 0, F, qdec, (uint64_t)qbytes, D);
    if (forked) HIPCHK(ctx, hipEventRecord(ctx->ev_f, F));
    if (coords) hipLaunchKernelGGL(k_dec_coords, dim3(2, n_chunks), dim3(64), 0, S, a->d_rfq, CH, D, B[DB_XV].as<uint32_t>(), B[DB_YV].as<uint32_t>());
    if ((HH.flags & H_N_POS) || ((HH.flags & H_QUAL_BY_COL) && !(HH.flags & H_DONT_QUAL))) {
        // position streams in POS_SEG-byte segments: summary -> link -> emit (see rfq_decode_kernels.h)
        // (grid sizes from the largest quality / N-position section: a file with raw qualities has no quality streams to walk)
        const bool bycol = (HH.flags & H_QUAL_BY_COL) && !(HH.flags & H_DONT_QUAL), hasn = (HH.flags & H_N_POS) != 0;
        const uint32_t nn = bycol ? std::min<uint32_t>(HH.n_normal, NPOS_SLOT) : 0u, nstr = HH.n_normal + 1;
        const uint32_t mq = nn ? g.max_stream / POS_SEG + 1 : 0u, mn = hasn ? g.max_npos / POS_SEG + 1 : 0u, maxseg = std::max(1u, std::max(mq, mn));
        const size_t nseg = (size_t)n_chunks * nstr * maxseg;
        HIPCHK(ctx, B[DB_SEGF].ensure(nseg + 16)); HIPCHK(ctx, B[DB_SEGA].ensure(nseg * 16 + 16)); HIPCHK(ctx, B[DB_SEGN].ensure((size_t)n_chunks * nstr * 4 + 16));
        HIPCHK(ctx, B[DB_SEGS].ensure(nseg + 16)); HIPCHK(ctx, B[DB_SEGP].ensure(nseg * 4 + 16));
        HIPCHK(ctx, hipMemsetAsync(B[DB_SEGN].p, 0, (size_t)n_chunks * nstr * 4, A));
#define RFQ_SUM_ARGS a->d_rfq, CH, D, R, (const uint64_t*)qbase, (const uint64_t*)sbase, qdec, sdec, B[DB_SEGF].as<uint8_t>(), B[DB_SEGA].as<int>(), B[DB_SEGN].as<uint32_t>(), maxseg, dst, (uint64_t)a->n
        if (nn) hipLaunchKernelGGL(k_dec_pos_sum, dim3(mq, nn, n_chunks), dim3(64), 0, A, RFQ_SUM_ARGS, 0u, nstr);
        if (hasn) hipLaunchKernelGGL(k_dec_pos_sum, dim3(mn, 1, n_chunks), dim3(64), 0, A, RFQ_SUM_ARGS, HH.n_normal, nstr);
#undef RFQ_SUM_ARGS
        hipLaunchKernelGGL(k_dec_pos_link, dim3((n_chunks * nstr + 255) / 256), dim3(256), 0, A, (const uint8_t*)B[DB_SEGF].as<uint8_t>(),
                (const int*)B[DB_SEGA].as<int>(),
                           (const uint32_t*)B[DB_SEGN].as<uint32_t>(), B[DB_SEGS].as<uint8_t>(), B[DB_SEGP].as<int>(), maxseg, n_chunks * nstr);
        if (forked) { HIPCHK(ctx, hipEventRecord(ctx->ev_mid, A)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_mid, 0)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_f, 0)); }
        hipLaunchKernelGGL(k_dec_unpack, dim3(bpc, n_chunks), dim3(256), 0, A, a->d_rfq, CH, R, (const uint64_t*)sbase, sdec, (uint64_t)a->n);
        if (nn) hipLaunchKernelGGL(k_dec_pos_emit, dim3(mq, nn, n_chunks), dim3(64), 0, S, a->d_rfq, CH, D, R, (const uint64_t*)qbase, (const uint64_t*)sbase, qdec, sdec,
                                   (const uint8_t*)B[DB_SEGS].as<uint8_t>(), (const int*)B[DB_SEGP].as<int>(), maxseg, (uint64_t)a->n, 0u, nstr);
        if (hasn) hipLaunchKernelGGL(k_dec_pos_emit, dim3(mn, 1, n_chunks), dim3(64), 0, A, a->d_rfq, CH, D, R, (const uint64_t*)qbase, (const uint64_t*)sbase, qdec,
                sdec,
                                     (const uint8_t*)B[DB_SEGS].as<uint8_t>(), (const int*)B[DB_SEGP].as<int>(), maxseg, (uint64_t)a->n, HH.n_normal, nstr);
    } else hipLaunchKernelGGL(k_dec_unpack, dim3(bpc, n_chunks), dim3(256), 0, A, a->d_rfq, CH, R, (const uint64_t*)sbase, sdec, (uint64_t)a->n);
    if (forked) { HIPCHK(ctx, hipEventRecord(ctx->ev_join, A)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_join, 0)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_f, 0)); }
    if (rle_h) hipLaunchKernelGGL(k_dec_rle, dim3(1, n_chunks), dim3(256), 0, S, a->d_rfq, CH, D, R, (const uint64_t*)qbase, qdec);
    hipLaunchKernelGGL(k_dec_except, dim3(bpc, n_chunks), dim3(256), 0, S, a->d_rfq, CH, D, R, (const uint64_t*)qbase, qdec);
    KCHK(ctx, "k_dec_streams");
    ctx->timer.end(S);
    E->qbase = qbase; E->sbase = sbase; E->qdec = qdec; E->sdec = sdec; E->qbytes = qbytes; E->sbytes = sbytes;
    return RFQ_OK;
}
// ---- the fused path of a range (rfq_decode_kernels.h "fused path"): the emitter builds qualities and bases tile by tile in LDS from the packed bytes and
// lists of coded positions.  It ends in k_dec_emit3 (no output tile, K reads per tile: the largest power of two whose qualities fit its tile).
// on: the range takes it; e3k: log2 K; n1big: the instantiation with the 13 KB name tile; shared_pieces: no chunk stores name pieces per read
struct FusedPlan { bool on; uint32_t e3k; bool n1big, shared_pieces; };
// Names FastqMeta::parse does not take apart and strand lines with text are stored per read: K then also goes by the chunks' average piece size, a fifth of the
// tile left for reads above the average, full tiles of 64 reads only (name1 has a second instantiation with a 13 KB tile: names of up to ~165 bytes on average,
// e.g. the configs[4] shape).  What does not fit - longer names, reads of more than 2000 bases, chunks of more than 4096 exception records, legacy run-length
// images - takes the ONE fallback: qualities and bases expanded in HBM, k_dec_emit.  A tile whose pieces turn out longer than the averages allowed for raises
// DE_E3_RETRY: the range is decoded again on the fallback (force_expanded: the retry cannot come back here), and the context remembers it for the ranges that
// follow until the next header is set or cleared.  Taken for files with few quality streams whose reads and exception lists fit a tile; RFQ_MATERIALISE=1 (the
// expanding decode of a streaming caller's non-final slices, on every call) forces the materialising path.
static FusedPlan plan_fused(const rfq_ctx* ctx, const DecRange& g, bool force_expanded) {
    const DevHeader& HH = ctx->h_hdr;
    const bool rle_h = !(HH.flags & (H_DONT_QUAL | H_QUAL_BY_COL));          // legacy run-length quality coding: k_dec_rle on the materialising path
    uint32_t e3k = 6; bool n1big = false;
    while (e3k >= 1 && ((uint64_t)g.max_len << e3k) > E3_QCAP) e3k--;
    if (g.per_read_pieces) {
        while (e3k >= 1 && ((uint64_t)g.piece_avg << e3k) > 204u) e3k--;
        const uint64_t need1 = ((uint64_t)g.piece_n1 << e3k) * 5u / 4u + 32u;
        if (need1 > ET_N1CAP) { if (e3k == 6 && need1 <= E3_N1BIG) n1big = true; else e3k = 0; }
    }
    const bool e3_ok = e3k >= (g.per_read_pieces ? 6u : 1u) && !(g.per_read_pieces && ctx->e3_pieces_failed);
    // (chunks of 2^30 bases and more: the list chain's saturating position sums - POS_ADV_MAX, dec/pos_lists.h - would no longer be exact)
    const bool on = !force_expanded && !ctx->opt.materialise && !rle_h && g.max_len <= 2000u && g.max_nrec <= 4096u && e3_ok && g.max_bases < (1u << 30) - 65536u;
    // (the per-read piece prefixes only where some chunk stores pieces per read: sequencer names leave none, and the stored-base prefix alone is 4 bytes per read instead of 16)
    return { on, e3k, n1big, E3_SHARED_OK && !g.per_read_pieces && !(HH.flags & H_DONT_QUAL) };
}
// what the position-list chain of a range left behind: the shape of its tables (B[DB_SEG*], B[DB_CELL], B[DB_NENT], B[DB_LOFF]), whether lists were built at
// all (a file without quality streams and N positions has none), and the stream the emitter has to wait for (join: the chain ran beside the main stream)
struct ListChain { uint32_t maxseg = 1, ncell = 1, nstr = 1, mq = 0, mn = 0, nn = 0, segb = POS2_SEG; bool hasn = false, built = false, join = false; hipStream_t aux = nullptr;
    // the grid of k_dec_pos_sum2 / k_dec_pos_list: the quality streams and, in the row behind them, the N-position stream in ONE launch - x for the longer of the two
    dim3 grid(uint32_t n_chunks) const { return dim3((maxseg + 3) / 4, nn + (hasn ? 1u : 0u), n_chunks); } };
// (an early return must not leave the chain running over buffers the next call reuses)
struct AuxJoin { rfq_ctx* c; bool armed; ~AuxJoin() { if (armed) (void)hipStreamSynchronize(c->aux); } };

// k_dec_pos_list for the quality streams and the N-position stream, one launch (the arena is whatever B[DB_PLIST] holds)
static void launch_pos_list(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const ListChain& L, hipStream_t LS) {
    DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>(); const DecStatus* dst = B[DB_STATUS].as<DecStatus>();
    const unsigned long long cap = B[DB_PLIST].cap / sizeof(plist_t);
#define RFQ_LIST_ARGS a->d_rfq, g.CH, D, (const uint8_t*)B[DB_SEGS].as<uint8_t>(), (const int*)B[DB_SEGP].as<int>(), (const uint32_t*)B[DB_SEGK].as<uint32_t>(), \
                      (const unsigned long long*)B[DB_LOFF].as<unsigned long long>(), B[DB_PLIST].as<plist_t>(), cap, B[DB_CELL].as<uint32_t>(), L.maxseg, L.ncell, (uint64_t)a->n
    hipLaunchKernelGGL(k_dec_pos_list, L.grid(g.n_chunks), dim3(256), 0, LS, RFQ_LIST_ARGS, L.nn, L.nstr, dst, L.segb);
#undef RFQ_LIST_ARGS
}
// The lists need nothing but the chunk table, so their chain (stream summaries, link, offsets, lists + cell index) starts at the top of a range on the second
// stream, beside read table, prefixes, coordinates and text lengths, and is joined in front of the emitter.  guard: armed from the fork on.
static int dec_list_chain(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, AuxJoin& guard, ListChain* L) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader& HH = ctx->h_hdr; const DevHeader* D = ctx->d_hdr.as<DevHeader>();
    DecStatus* dst = B[DB_STATUS].as<DecStatus>(); const DChunk* CH = g.CH; const uint32_t n_chunks = g.n_chunks;
    const bool bycol_h = (HH.flags & H_QUAL_BY_COL) && !(HH.flags & H_DONT_QUAL);
    L->nstr = HH.n_normal + 1; L->hasn = (HH.flags & H_N_POS) != 0; L->nn = bycol_h ? std::min<uint32_t>(HH.n_normal, NPOS_SLOT) : 0u;
    if (!L->nn && !L->hasn) return RFQ_OK;
    const bool forked = ctx->aux_ready(); hipStream_t A = forked ? ctx->aux : S;
    if (forked) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(A, ctx->ev_fork, 0)); guard.armed = true; }
    L->segb = ctx->opt.pos_seg ? (uint32_t)ctx->opt.pos_seg : (std::max(g.max_one, g.max_npos) >= 32768u ? POS2_SEG_BIG : POS2_SEG);
    L->mq = L->nn ? g.max_one / L->segb + 1 : 0u; L->mn = L->hasn ? g.max_npos / L->segb + 1 : 0u; L->maxseg = std::max(1u, std::max(L->mq, L->mn));
    L->ncell = g.max_bases / POS2_CELL + 2;
    const size_t nst = (size_t)n_chunks * L->nstr, nseg = nst * L->maxseg, ncl = nst * L->ncell;
    HIPCHK(ctx, B[DB_SEGF].ensure(nseg + 16)); HIPCHK(ctx, B[DB_SEGA].ensure(nseg * 32 + 16)); HIPCHK(ctx, B[DB_SEGN].ensure(nst * 4 + 16));
    HIPCHK(ctx, B[DB_SEGS].ensure(nseg + 16)); HIPCHK(ctx, B[DB_SEGP].ensure(nseg * 4 + 16)); HIPCHK(ctx, B[DB_SEGK].ensure(nseg * 4 + 16));
    HIPCHK(ctx, B[DB_CELL].ensure(ncl * 4 + 16));
    HIPCHK(ctx, B[DB_NENT].ensure(nst * 4 + 16)); HIPCHK(ctx, B[DB_LOFF].ensure(nst * 8 + 16));
    // the arena of the position lists: a position belongs to at most one stream, the coded ones are a few percent of the bases; if a
    // file needs more than the arena holds, k_dec_pos_list leaves it alone and decode_range repeats the pass with the right size
    // (an entry per eight bases to begin with - half a byte per base; a NovaSeq-binned file codes one position in twelve.  A file that codes more
    // - forty quality values code most positions - runs the list pass a second time, once per context: the arena keeps its size.  Two bytes per base
    // up front would be 6.7 GB on 2 x 4 GB of text)
    if (B[DB_PLIST].ensure((size_t)(g.bases / 8 + 1024) * sizeof(plist_t)) != hipSuccess) { (void)hipGetLastError();
            HIPCHK(ctx, B[DB_PLIST].ensure((size_t)(g.bases / 32 + 1024) * sizeof(plist_t))); }
    { ClearList z; memset(&z, 0, sizeof z); z.add(B[DB_SEGN].p, nst * 4, 0u); z.add(B[DB_NENT].p, nst * 4, 0u); z.add(B[DB_CELL].p, ncl * 4, 0xFFFFFFFFu); clear_list(A, z); }
#define RFQ_SUM2_ARGS a->d_rfq, CH, D, B[DB_SEGF].as<uint8_t>(), B[DB_SEGA].as<int>(), B[DB_SEGN].as<uint32_t>(), L->maxseg, dst, (uint64_t)a->n
    hipLaunchKernelGGL(k_dec_pos_sum2, L->grid(n_chunks), dim3(256), 0, A, RFQ_SUM2_ARGS, L->nn, L->nstr, L->segb);
#undef RFQ_SUM2_ARGS
    hipLaunchKernelGGL(k_dec_pos_link2, dim3((uint32_t)((nst + 3) / 4)), dim3(256), 0, A, (const uint8_t*)B[DB_SEGF].as<uint8_t>(), (const int*)B[DB_SEGA].as<int>(),
                       (const uint32_t*)B[DB_SEGN].as<uint32_t>(), B[DB_SEGS].as<uint8_t>(), B[DB_SEGP].as<int>(), B[DB_SEGK].as<uint32_t>(), B[DB_NENT].as<uint32_t>(),
                       L->maxseg, (uint32_t)nst, CH, L->nstr, dst);
    hipLaunchKernelGGL(k_dec_pos_off, dim3(1), dim3(256), 0, A, (const uint32_t*)B[DB_NENT].as<uint32_t>(), B[DB_LOFF].as<unsigned long long>(), (uint32_t)nst, dst);
    launch_pos_list(ctx, a, g, *L, A);
    L->built = true; L->join = forked; L->aux = A;
    KCHK(ctx, "k_dec_pos_*");
    return RFQ_OK;
}
// fused read table: chunk-local prefixes made where the per-read values are made (k_dec_readtab2): no per-read scan inputs, no batch-wide scans, no read-back
// here - the status word is looked at with the next one, the range's bases are the walk's 64-bit total.  R.len / R.ov / R.mid are the caller's.
static int dec_table_fused(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const FusedPlan& P, const DReadTab& R, DFused* F) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    const size_t nr = (size_t)g.n_reads + 2, nc = (size_t)g.n_chunks + 2;
    HIPCHK(ctx, B[DB_PQL].ensure((nr + nc) * 4)); HIPCHK(ctx, B[DB_TPL].ensure(nr * 8));
    if (!P.shared_pieces) HIPCHK(ctx, B[DB_PVL].ensure((nr + nc) * 16));
    HIPCHK(ctx, B[DB_CTEXT].ensure(nc * 16)); HIPCHK(ctx, B[DB_TBASE].ensure(nc * 16)); HIPCHK(ctx, B[DB_SCAN].ensure((nc / SCAN_TILE + 2) * 16 + 1024));
    HIPCHK(ctx, B[DB_SDL].ensure((nr + nc) * 4));
    U4* const pvl = P.shared_pieces ? (U4*)nullptr : B[DB_PVL].as<U4>();
    F->len = R.len; F->ov = R.ov; F->pql = B[DB_PQL].as<uint32_t>(); F->pvl = pvl; F->sdl = B[DB_SDL].as<uint32_t>();
    F->tpl = B[DB_TPL].as<uint2>(); F->tbase = B[DB_TBASE].as<U4>(); F->mid = R.mid;
    hipLaunchKernelGGL(k_dec_readtab2, dim3(g.n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, ctx->d_hdr.as<DevHeader>(), R.len, R.ov, B[DB_PQL].as<uint32_t>(), pvl,
                       B[DB_SDL].as<uint32_t>(), B[DB_STATUS].as<DecStatus>());
    KCHK(ctx, "k_dec_readtab2");
    ctx->timer.end(S);
    return RFQ_OK;
}
// fused text lengths, timer stage "streams" (the list chain has been running beside it since the top of the range): the coordinate decoder, the lengths of
// every read's text (k_dec_textlen2), where every chunk's text starts (entry n_chunks of B[DB_TBASE]: the totals)
static int dec_textlen_fused(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const DReadTab& R) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>();
    ctx->timer.begin("streams", S);
    hipLaunchKernelGGL(k_dec_coords, dim3(2, g.n_chunks), dim3(64), 0, S, a->d_rfq, g.CH, D, B[DB_XV].as<uint32_t>(), B[DB_YV].as<uint32_t>());
    KCHK(ctx, "k_dec_coords");
    hipLaunchKernelGGL(k_dec_textlen2, dim3(g.n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, D, (const uint32_t*)R.len, R.mid, (const uint32_t*)B[DB_XV].as<uint32_t>(),
                       (const uint32_t*)B[DB_YV].as<uint32_t>(), a->split_pe ? 1 : 0, B[DB_TPL].as<uint2>(), B[DB_CTEXT].as<U4>(), B[DB_STATUS].as<DecStatus>());
    KCHK(ctx, "k_dec_textlen2");
    scan_exclusive<U4>(S, B[DB_CTEXT].as<U4>(), B[DB_TBASE].as<U4>(), g.n_chunks, B[DB_SCAN].as<U4>(), 1);
    return RFQ_OK;
}
// k_dec_emit3 into o1 / o2.  list_cap != 0: the speculative launch - the kernel looks at the status itself (dec/emit_tiles.h) -, 0: the host has looked.
static void launch_emit3(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const FusedPlan& P, const ListChain& L, const DFused& F,
                         uint8_t* o1, uint64_t cap1, uint8_t* o2, uint64_t cap2, unsigned long long list_cap) {
    DBuf* B = ctx->b; const bool hasn = (ctx->h_hdr.flags & H_N_POS) != 0;
    // (25 KB of LDS: six workgroups per CU; four with the large name tile)
    const uint32_t K = 1u << P.e3k, bx = grid_x_for(g.n_chunks, (std::max(g.max_reads, 1u) + K - 1) / K, (P.n1big ? 4u : 6u) * ctx->n_cu);
    const dim3 grid(bx, g.n_chunks);
#define RFQ_EMIT3_ARGS a->d_rfq, g.CH, ctx->d_hdr.as<DevHeader>(), F, (uint64_t)a->n, a->split_pe ? 1 : 0, o1, cap1, o2, cap2, B[DB_STATUS].as<DecStatus>(), \
                       (const plist_t*)B[DB_PLIST].as<plist_t>(), (const unsigned long long*)B[DB_LOFF].as<unsigned long long>(), (const uint32_t*)B[DB_NENT].as<uint32_t>(), \
                       (const uint32_t*)B[DB_CELL].as<uint32_t>(), L.ncell, L.nstr, P.e3k, list_cap
    if (P.n1big) {
        if (hasn) hipLaunchKernelGGL((k_dec_emit3<false, E3_N1BIG>), grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
        else hipLaunchKernelGGL((k_dec_emit3<true, E3_N1BIG>), grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
    } else if (F.pvl == nullptr) {                                         // (every chunk shares its name pieces among its reads: the instantiation without per-read piece prefixes)
        if (hasn) hipLaunchKernelGGL((k_dec_emit3<false, ET_N1CAP, true>), grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
        else hipLaunchKernelGGL((k_dec_emit3<true, ET_N1CAP, true>), grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
    }
    else if (hasn) hipLaunchKernelGGL(k_dec_emit3<false>, grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
    else hipLaunchKernelGGL(k_dec_emit3<true>, grid, dim3(256), 0, ctx->stream, RFQ_EMIT3_ARGS);
#undef RFQ_EMIT3_ARGS
}
// RfqCodec::decodeChunk + Read::toString for the chunks of one range (reads, bases and text of a range are placed by 32-bit prefix sums).
// out: caller buffers (16-byte aligned) or null = the context's own result buffers; *T (set on RFQ_OK only) = where the text of R1 / R2 went.
// force_expanded: the retry of a range whose fused path gave up - straight to the expanded path, whatever made it give up (the retry must terminate by
// construction, not because a flag happens to be honoured)
struct DecDst { uint8_t* p[2]; uint64_t cap[2]; };
struct DecText { uint8_t* p[2]; size_t n[2]; uint64_t bases; };
static int decode_range(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const DecDst& out, DecText* T, bool force_expanded = false) {
    uint8_t* const out1 = out.p[0]; uint8_t* const out2 = out.p[1]; uint64_t nbases = 0;
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>();
    DecStatus* dst = B[DB_STATUS].as<DecStatus>(); DecStatus hs;
    const uint32_t n_chunks = g.n_chunks, n_reads = g.n_reads, max_reads = std::max(g.max_reads, 1u);
    const int split = a->split_pe ? 1 : 0;
    HIPCHK(ctx, hipMemsetAsync(dst, 0, sizeof(DecStatus), S));
    const FusedPlan P = plan_fused(ctx, g, force_expanded);
    ListChain L; AuxJoin aux_guard = { ctx, false };
    if (P.on) { const int rc = dec_list_chain(ctx, a, g, aux_guard, &L); if (rc) return rc; }
    // ---- read table + prefixes, streams, text lengths
    ctx->timer.begin("read_table", S);
    const size_t nr = (size_t)n_reads + 2;
    HIPCHK(ctx, B[DB_LEN].ensure(nr * 4)); HIPCHK(ctx, B[DB_OV].ensure(nr * 4));
    HIPCHK(ctx, B[DB_XV].ensure(nr * 4)); HIPCHK(ctx, B[DB_YV].ensure(nr * 4)); HIPCHK(ctx, B[DB_MID].ensure(nr * 40));
    DReadTab R; memset(&R, 0, sizeof R); DFused F; memset(&F, 0, sizeof F); DecExpanded E; memset(&E, 0, sizeof E);
    R.len = B[DB_LEN].as<uint32_t>(); R.ov = B[DB_OV].as<int32_t>(); R.mid = B[DB_MID].as<uint8_t>();
    if (P.on) {
        int rc = dec_table_fused(ctx, a, g, P, R, &F);
        if (!rc) rc = dec_textlen_fused(ctx, a, g, R);
        if (rc) return rc;
        nbases = g.bases;
    } else {
        uint32_t total_bases = 0; U4 pv_tot; memset(&pv_tot, 0, sizeof pv_tot);
        int rc = dec_table_expanded(ctx, a, g, R, true, &total_bases, &pv_tot);
        if (!rc) rc = dec_streams_expanded(ctx, a, g, R, total_bases, pv_tot, true, &E);
        if (rc) return rc;
        nbases = total_bases;
        ctx->timer.begin("textlen", S);
        hipLaunchKernelGGL(k_dec_textlen, dim3((max_reads + 255) / 256, n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, D, R, (const uint32_t*)B[DB_XV].as<uint32_t>(),
                           (const uint32_t*)B[DB_YV].as<uint32_t>(), split, dst);
        scan_exclusive<U4>(S, R.tin, R.tp, n_reads, B[DB_SCAN].as<U4>(), 1);
    }
    if (L.join) { HIPCHK(ctx, hipEventRecord(ctx->ev_join, L.aux)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_join, 0)); }
    aux_guard.armed = false;       // (everything below is ordered behind the chain on the main stream)
    // Speculative emit (fused path, the caller's output buffers, lists that were built): the emitter is launched WITHOUT the read-back below - it stops itself on what the
    // checks would have stopped at (k_dec_emit3: list_cap) -, and the host looks once, behind it: one round trip less per range (~35 us: 3 % of a 1 GB decode).
    bool emitted = P.on && L.built && out1 && (!a->split_pe || out2) && !((uintptr_t)out1 & 15u) && !(out2 && ((uintptr_t)out2 & 15u)) && !ctx->opt.no_spec;
    if (emitted) {
        ctx->timer.end(S);
        ctx->timer.begin("emit", S);
        launch_emit3(ctx, a, g, P, L, F, out1, out.cap[0], out2, out.cap[1], B[DB_PLIST].cap / sizeof(plist_t));
        KCHK(ctx, "k_dec_emit");
        ctx->timer.end(S);
    }
    // ---- the verdict: once in front of the emitter (unless it went ahead), once behind it
    U4 tt; HIPCHK(ctx, ctx->fetch(&tt, P.on ? B[DB_TBASE].as<U4>() + n_chunks : R.tp + n_reads, 16, S));
    uint8_t *o1, *o2;
    for (;;) {
        HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
        // (k_dec_readtab2's verdict, a bit of its own: the list chain's DE_CORRUPT means the quality buffer - the same two messages as on the expanded path)
        if (hs.err & DE_CORRUPT_OV) return rfq_fail(ctx, RFQ_E_FORMAT, "corrupt overlap buffer");
        // once more, expanded.  DE_LIST_ALIAS: a stream codes positions far beyond its chunk's length table (k_dec_pos_link2): 16-bit list entries would alias.
        // DE_E3_RETRY: per-read name pieces that did not fit a tile of k_dec_emit3 - files like this one: the ranges that follow go straight to the expanded path
        if (P.on && (hs.err & (DE_LIST_ALIAS | DE_E3_RETRY))) {
            if ((hs.err & DE_E3_RETRY) && g.per_read_pieces) ctx->e3_pieces_failed = true;
            return decode_range(ctx, a, g, out, T, true);
        }
        if (hs.err & DE_CORRUPT) return rfq_fail(ctx, RFQ_E_FORMAT, "corrupt quality buffer");
        if (L.built && hs.list_need > B[DB_PLIST].cap / sizeof(plist_t)) {       // the lists did not fit the arena: now that their size is known, build them
            if (emitted) { emitted = false; ctx->timer.begin("streams", S); }        // (the speculative emitter left at once: the ordinary order from here on)
            HIPCHK(ctx, B[DB_PLIST].ensure((size_t)(hs.list_need + 1024) * sizeof(plist_t)));
            launch_pos_list(ctx, a, g, L, S);
            KCHK(ctx, "k_dec_pos_list");
        }
        // text prefix sums are 32-bit: one decode call emits < 4 GiB per output stream
        hs.text1 = hs.text2 = 0; for (int i = 0; i < 64; i++) { hs.text1 += hs.text_slots[0][i]; hs.text2 += hs.text_slots[1][i]; }
        if (hs.text1 >= 0xFFFFFFF0ull || hs.text2 >= 0xFFFFFFF0ull) return RFQ_RANGE_TOO_BIG;       // (the caller decodes the range in two halves)
        if ((out1 && ((uintptr_t)out1 & 15u)) || (out2 && ((uintptr_t)out2 & 15u))) return rfq_fail(ctx, RFQ_E_ARG, "output device pointers must be 16-byte aligned");
        uint64_t cap1, cap2;
        if (out1) { o1 = out1; cap1 = out.cap[0]; } else { HIPCHK(ctx, ctx->out_fq1.ensure((size_t)tt.a + 64)); o1 = ctx->out_fq1.as<uint8_t>(); cap1 = ctx->out_fq1.cap; }
        if (out2) { o2 = out2; cap2 = out.cap[1]; } else { HIPCHK(ctx, ctx->out_fq2.ensure((size_t)tt.b + 64)); o2 = ctx->out_fq2.as<uint8_t>(); cap2 = ctx->out_fq2.cap; }
        if (emitted) break;
        ctx->timer.end(S);
        ctx->timer.begin(P.on ? "emit" : "emit_expanded", S);              // the emitter alone: the path's largest kernel (bench.py roofline)
        if (P.on) launch_emit3(ctx, a, g, P, L, F, o1, cap1, o2, cap2, 0ull);
        else {
            const uint32_t bx = grid_x_for(n_chunks, (max_reads + ET_READS - 1) / ET_READS, 4u * ctx->n_cu);   // (39 KB of LDS: four workgroups per CU)
            hipLaunchKernelGGL(k_dec_emit, dim3(bx, n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, D, R, (const uint64_t*)E.qbase, (const uint64_t*)E.sbase,
                               (const uint8_t*)E.qdec, (const uint8_t*)E.sdec, (uint64_t)E.qbytes, (uint64_t)E.sbytes, (uint64_t)a->n, split, o1, cap1, o2, cap2, dst);
        }
        KCHK(ctx, "k_dec_emit");
        ctx->timer.end(S);
        emitted = true;
    }
    ctx->timer.collect();
    if (hs.err & (1u << 31)) return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffer too small: need %u / %u bytes", tt.a, tt.b);
    *T = DecText{ { o1, o2 }, { tt.a, split ? tt.b : 0u }, nbases };
    return RFQ_OK;
}

// the range of chunks [CH, CH + n_chunks) with the walk's image-wide maxima
static DecRange range_of(const DecStatus& hs, const DChunk* CH, uint32_t n_chunks, uint64_t reads, uint64_t bases) {
    DecRange g; g.CH = CH; g.n_chunks = n_chunks; g.n_reads = (uint32_t)reads; g.max_reads = hs.max_reads; g.bases = bases;
    take_maxima(g, hs); return g;
}

// what every decode call does first: the device, the stage timers, the header (parsed from the image and set, or the one set before);
// *start = where the image's chunks begin
static int dec_open(rfq_ctx* ctx, const rfq_decode_args* a, uint64_t* start) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->timer.reset();
    ctx->pend.clear(); ctx->pin_used = 0;                                   // (read-backs an earlier call left behind on an error path)
    *start = 0;
    if (a->has_header) {
        uint8_t hb[RFQ_HEADER_MAX]; const size_t take = std::min<size_t>(a->n, sizeof hb);
        if (take) HIPCHK(ctx, hipMemcpy(hb, a->d_rfq, take, hipMemcpyDeviceToHost));
        int rc = rfq_upload_header(ctx, hb, take);
        if (rc) return rc;
        *start = ctx->h_hdr.len;
    } else if (!ctx->have_hdr) return rfq_fail(ctx, RFQ_E_STATE, "decode without a header: pass has_header=1 or call rfq_set_header first");
    return RFQ_OK;
}
// the chunk chain of the image: the caller's chunk index (verified), guess-and-verify or the exact walk, the verifying parse behind it.
// hs: chunks, reads, bases, the longest read / stream / chunk, consumed - exact on every path
static int dec_walk(rfq_ctx* ctx, const rfq_decode_args* a, uint64_t start, DecStatus& hs) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader& HH = ctx->h_hdr;
    if (HH.read_len_bytes != 1 && HH.read_len_bytes != 2 && HH.read_len_bytes != 4) return rfq_fail(ctx, RFQ_E_DATA,
            "header incorrect: read length bytes should be 1/2/4");
    const DevHeader* D = ctx->d_hdr.as<DevHeader>();

    // ---- walk the chunk chain
    ctx->timer.begin("walk", S);
    HIPCHK(ctx, B[DB_STATUS].ensure(sizeof(DecStatus)));
    DecStatus* dst = B[DB_STATUS].as<DecStatus>();
    uint32_t cap = (uint32_t)std::max<size_t>(B[DB_CHUNKS].cap / sizeof(DChunk), 4096);
    // the chunk starts: the caller's chunk index (verified below); else guess-and-verify (k_dec_gw_*: an index made on the device, verified the same
    // way); else the exact serial walk (one wave, a full parse per chunk: foreign writers, corrupt images)
    bool use_table = a->h_chunk_off && a->n_chunk_off && a->h_chunk_off[0] == start && a->h_chunk_off[a->n_chunk_off] <= a->n;
    bool guess = !use_table && !ctx->opt.walk_exact;                         // (RFQ_WALK=exact: straight to the serial walk; tests run both)
    for (;;) {
        if (use_table && a->n_chunk_off + 1u > cap) cap = a->n_chunk_off + 1u;
        HIPCHK(ctx, B[DB_CHUNKS].ensure((size_t)cap * sizeof(DChunk)));
        ClearList wz; memset(&wz, 0, sizeof wz); wz.add(dst, sizeof(DecStatus), 0u);       // (the walk's fills in one launch: status, candidates, the "no candidate" count)
        const bool indexed = use_table || guess;                             // chunk starts that have to verify
        if (use_table) {
            const size_t tb = ((size_t)a->n_chunk_off + 1) * 8;
            clear_list(S, wz);
            HIPCHK(ctx, B[DB_OFFT].ensure(tb));
            HIPCHK(ctx, hipMemcpyAsync(B[DB_OFFT].p, a->h_chunk_off, tb, hipMemcpyHostToDevice, S));
            hipLaunchKernelGGL(k_dec_table, dim3(1), dim3(256), 0, S, a->d_rfq, (uint64_t)a->n, (const uint64_t*)B[DB_OFFT].as<uint64_t>(), a->n_chunk_off,
                    B[DB_CHUNKS].as<DChunk>(), dst);
        } else if (guess) {
            HIPCHK(ctx, B[DB_OFFT].ensure(((size_t)cap + 2) * 8));
            HIPCHK(ctx, B[DB_GWCAND].ensure(GW_SEGS * 8 + 64)); HIPCHK(ctx, B[DB_GWLIST].ensure((size_t)GW_SEGS * GW_LCAP * 8));
                    HIPCHK(ctx, B[DB_GWCNT].ensure(GW_SEGS * 4 + 64)); HIPCHK(ctx, B[DB_GWLAND].ensure(GW_SEGS * 8 + 64));
            unsigned long long* cand = B[DB_GWCAND].as<unsigned long long>(); uint32_t* gbad = B[DB_GWCNT].as<uint32_t>() + GW_SEGS;
            wz.add(cand, GW_SEGS * 8, 0xFFFFFFFFu); wz.add(gbad, 4, 0u); clear_list(S, wz);
            // (a segment is 16 chunks or more: no use in more segments than 64 KB pieces; RFQ_GW_SHIFT: test aid)
            const uint32_t mseg = (uint32_t)std::min<uint64_t>(GW_SEGS, std::max<uint64_t>(1, (a->n - start) >> ctx->opt.gw_shift));
            if (mseg > 1) hipLaunchKernelGGL(k_dec_gw_find, dim3(16, mseg - 1), dim3(256), 0, S, a->d_rfq, (uint64_t)a->n, start, D, cand, mseg);
            hipLaunchKernelGGL(k_dec_gw_walk, dim3(mseg), dim3(64), 0, S, a->d_rfq, (uint64_t)a->n, start, D, (const unsigned long long*)cand,
                    B[DB_GWLIST].as<unsigned long long>(), B[DB_GWCNT].as<uint32_t>(), B[DB_GWLAND].as<unsigned long long>(), gbad, mseg, a->final ? 1 : 0);
            hipLaunchKernelGGL(k_dec_gw_stitch, dim3(1), dim3(1024), 0, S, a->d_rfq, (uint64_t)a->n, start, D, (const unsigned long long*)cand,
                    (const unsigned long long*)B[DB_GWLIST].as<unsigned long long>(),
                               (const uint32_t*)B[DB_GWCNT].as<uint32_t>(), (const unsigned long long*)B[DB_GWLAND].as<unsigned long long>(), (const uint32_t*)gbad, B[DB_OFFT].as<uint64_t>(), cap, dst, mseg);
            hipLaunchKernelGGL(k_dec_table, dim3(1), dim3(256), 0, S, a->d_rfq, (uint64_t)a->n, (const uint64_t*)B[DB_OFFT].as<uint64_t>(), 0xFFFFFFFFu,
                    B[DB_CHUNKS].as<DChunk>(), dst);
        }
        else { clear_list(S, wz); hipLaunchKernelGGL(k_dec_walk, dim3(1), dim3(64), 0, S, a->d_rfq, (uint64_t)a->n, start, D, B[DB_CHUNKS].as<DChunk>(), cap, dst, a->final ? 1 : 0); }
        KCHK(ctx, "k_dec_walk");
        // the verifying parse rides behind the index without a host round trip in between (its grid covers the first
        // PARSE_AHEAD chunks; the walk's own verdict is in the status words it reads)
        const uint32_t PARSE_AHEAD = use_table ? std::max(a->n_chunk_off, 1u) : 4096u;
        if (indexed) {
            hipLaunchKernelGGL(k_dec_parse, dim3(std::min(cap, PARSE_AHEAD)), dim3(64), 0, S, a->d_rfq, (uint64_t)a->n, D, B[DB_CHUNKS].as<DChunk>(), dst, 0u);
            hipLaunchKernelGGL(k_dec_summary, dim3(1), dim3(256), 0, S, (const DChunk*)B[DB_CHUNKS].as<DChunk>(), dst, 0u, std::min(cap, PARSE_AHEAD));
            KCHK(ctx, "k_dec_parse");
        }
        HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
        if (use_table) {
            // the table must cover whole chunks up to the end of the image (or up to a tail too short to be a chunk): anything else walks
            // (a range that does not end the image may end inside a chunk: whole chunks in front of it are all a table has to cover there)
            if (hs.pad || (hs.consumed != a->n && a->n - hs.consumed >= 18 && (a->final || hs.n_chunks == 0))) { use_table = false; guess = !ctx->opt.walk_exact;
                    continue; }
            break;
        }
        if (hs.overflow) { cap = hs.n_chunks + 1024; continue; }
        // (the exact walk does not look into the quality payloads: such images take the materialising path)
        if (!indexed) { hs.max_nrec = 0xFFFFFFFFu; hs.max_one = hs.max_stream; hs.per_read_pieces = 1; hs.piece_avg = 0xFFFFu; hs.piece_n1 = 0xFFFFu; break; }
        if (hs.pad) { guess = false; continue; }                           // the guessed index did not verify (foreign writer / corrupt image): walk it properly
        if (hs.n_chunks > PARSE_AHEAD) {
            hipLaunchKernelGGL(k_dec_parse, dim3(hs.n_chunks - PARSE_AHEAD), dim3(64), 0, S, a->d_rfq, (uint64_t)a->n, D, B[DB_CHUNKS].as<DChunk>(), dst, PARSE_AHEAD);
            hipLaunchKernelGGL(k_dec_summary, dim3(1), dim3(256), 0, S, (const DChunk*)B[DB_CHUNKS].as<DChunk>(), dst, PARSE_AHEAD, hs.n_chunks - PARSE_AHEAD);
            KCHK(ctx, "k_dec_parse");
            DecStatus h2; HIPCHK(ctx, ctx->fetch(&h2, dst, sizeof h2, S));
            HIPCHK(ctx, ctx->fetch_sync(S));
            if (h2.pad) { guess = false; continue; }
            take_maxima(hs, h2); memcpy(hs.base_slots, h2.base_slots, sizeof hs.base_slots);
        }
        // let the exact walk decide about a trailing partial chunk (a range that does not end the image may end inside one)
        if (hs.consumed != a->n && a->n - hs.consumed >= 18 && (a->final || hs.n_chunks == 0)) { guess = false; continue; }
        break;
    }
    if (ctx->opt.trace) fprintf(stderr, "[rfq] chunk starts: %s, %u chunks\n", use_table ? "caller's index" : (guess ? "guess-and-verify" : "exact walk"), hs.n_chunks);
    ctx->timer.end(S);
    if (hs.err & DE_CORRUPT) return rfq_fail(ctx, RFQ_E_FORMAT, "truncated or corrupt rfq chunk at byte %llu", (unsigned long long)hs.consumed);
    return RFQ_OK;
}

// ---- what text, rows and names share: the walked image and the loop over its ranges
// rfq_decode_rows_args / rfq_decode_names_args as the text decode's arguments, which the walk and the stages of a range take (split_pe = 0, bug_compat = 0:
// Repaq::decompress order, nothing lost)
template <class A> static rfq_decode_args dec_view(const A* x) {
    rfq_decode_args a; memset(&a, 0, sizeof a);
    a.d_rfq = x->d_rfq; a.n = x->n; a.has_header = x->has_header; a.final = x->final; a.h_chunk_off = x->h_chunk_off; a.n_chunk_off = x->n_chunk_off;
    return a;
}
// hs: the walk's status; CHm: the chunk table on the device; bases: the 64-bit total of the read lengths - bases, qualities and text are placed by 32-bit
// prefix sums (a corrupt length table must be refused before any buffer is sized from a wrapped sum); empty: an empty .rfq, nothing walked;
// hc: the host copy of the chunk table, made once for whoever asks first (dec_host_table: bug_compat, ranges)
struct DecImage { uint64_t start; DecStatus hs; DChunk* CHm; uint32_t n_chunks; uint64_t reads, bases; bool empty; std::vector<DChunk> hc; };
static int dec_image(rfq_ctx* ctx, const rfq_decode_args* a, DecImage* img) {
    img->start = 0; memset(&img->hs, 0, sizeof img->hs); img->empty = a->n == 0 && a->has_header;
    if (img->empty) { HIPCHK(ctx, hipSetDevice(ctx->device)); ctx->timer.reset(); }      // (no header to parse, no chunk to walk)
    else {
        int rc = dec_open(ctx, a, &img->start); if (rc) return rc;
        if (a->split_pe && !(ctx->h_hdr.flags & H_PAIRED)) return rfq_fail(ctx, RFQ_E_DATA, "The input RFQ file was encoded by single-end FASTQ, you should not specify <out2>");
        rc = dec_walk(ctx, a, img->start, img->hs); if (rc) return rc;
    }
    img->CHm = ctx->b[DB_CHUNKS].as<DChunk>(); img->n_chunks = img->hs.n_chunks; img->reads = img->hs.total_reads;
    img->bases = 0; for (int i = 0; i < 16; i++) img->bases += img->hs.base_slots[i];
    return RFQ_OK;
}
static int dec_host_table(rfq_ctx* ctx, DecImage& img) {
    if (img.hc.size() == img.n_chunks) return RFQ_OK;
    img.hc.resize(img.n_chunks); HIPCHK(ctx, hipMemcpy(img.hc.data(), img.CHm, (size_t)img.n_chunks * sizeof(DChunk), hipMemcpyDeviceToHost));
    return RFQ_OK;
}
// the range of one span: its reads and bases summed from the host copy of the chunk table, its chunks' read bases made relative to it (k_dec_rebase)
static int span_range(rfq_ctx* ctx, const DecImage& img, const ChunkSpan& r, DecRange* g, uint64_t* reads) {
    uint64_t rd = 0, rbases = 0; for (uint32_t c = r.c0; c < r.c1; c++) { rd += img.hc[c].reads; rbases += img.hc[c].bases; }
    hipLaunchKernelGGL(k_dec_rebase, dim3((r.c1 - r.c0 + 255) / 256), dim3(256), 0, ctx->stream, img.CHm + r.c0, r.c1 - r.c0, img.hc[r.c0].rbase_abs);
    KCHK(ctx, "k_dec_rebase");
    *g = range_of(img.hs, img.CHm + r.c0, r.c1 - r.c0, rd, rbases); *reads = rd;
    return RFQ_OK;
}
// body(range, span, whole) over the image.  One pass where the image fits one (whole = true: the chunk table as the walk left it, the stage timers the
// caller's to collect); else - and when that pass says RFQ_RANGE_TOO_BIG, or the caller names the pieces to decode (bug_compat) - range by range (dec/ranges.h;
// RFQ_SLICE_BASES: test aid - ranges of that many bases, so that this runs on small images), the stage times of every range summed into `sums` behind the
// walk's and whatever a failed one-pass attempt got through.  A non-empty `sums` says that ranges ran (and run from then on): the caller publishes it.
// A range the body calls too big is halved, a single chunk that is too big fails with `too_big`.  plan_ranges cuts at a pass's limits of reads and
// bases, so only a single chunk can exceed those: what does get halved is a range whose text reaches 4 GiB.
template <class Body>
static int dec_each_range(rfq_ctx* ctx, DecImage& img, const std::vector<ChunkSpan>* pieces, StageSums& sums, const char* too_big, Body body) {
    if (!img.n_chunks) return RFQ_OK;
    const uint64_t slice_env = ctx->opt.slice_bases, slice_bases = slice_env ? slice_env : 1500000000ull, one_pass = slice_env ? slice_env : RANGE_MAX_BASES;
    if (!pieces && sums.v.empty() && img.bases < one_pass && img.reads < RANGE_MAX_READS) {
        const int rc = body(range_of(img.hs, img.CHm, img.n_chunks, img.reads, img.bases), ChunkSpan{ 0, img.n_chunks, false }, true);
        if (rc != RFQ_RANGE_TOO_BIG) return rc;
    }
    { const int rc = dec_host_table(ctx, img); if (rc) return rc; }
    RangeQueue todo = plan_ranges(pieces ? *pieces : std::vector<ChunkSpan>{ { 0, img.n_chunks, false } }, img.hc.data(), slice_bases);
    if (sums.v.empty()) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); ctx->timer.collect(); sums.add(ctx->timer); }
    for (ChunkSpan r; todo.next(&r);) {
        DecRange g; uint64_t reads = 0;
        int rc = span_range(ctx, img, r, &g, &reads); if (rc) return rc;
        ctx->timer.reset();
        rc = reads >= RANGE_MAX_READS ? RFQ_RANGE_TOO_BIG : body(g, r, false);
        if (rc == RFQ_RANGE_TOO_BIG) { if (!todo.halve(r)) return rfq_fail(ctx, RFQ_E_ARG, "%s", too_big); continue; }
        if (rc) return rc;
        ctx->timer.collect(); sums.add(ctx->timer);
    }
    return RFQ_OK;
}
// the stage times of a call: the one pass's, or the sums over its ranges
static void dec_timings(rfq_ctx* ctx, const StageSums& sums) { if (sums.v.empty()) ctx->timer.collect(); else sums.publish(ctx->timer); }

extern "C" int rfq_decode_batch(rfq_ctx* ctx, const rfq_decode_args* a, rfq_decode_result* res) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (a->n && !a->d_rfq) return rfq_fail(ctx, RFQ_E_ARG, "null rfq pointer");
    if (a->n == 0 && a->has_header) {
        // an empty .rfq: every read of RfqHeader::read fails and the constructor's defaults stand (valid magic, flags 0;
        // src/rfqheader.cpp:7-17,19-43), no chunk follows: the reference writes an empty FASTQ
        if (a->split_pe) return rfq_fail(ctx, RFQ_E_DATA, "The input RFQ file was encoded by single-end FASTQ, you should not specify <out2>");
        return RFQ_OK;
    }
    DecImage img; { const int rc = dec_image(ctx, a, &img); if (rc) return rc; }
    res->consumed = (size_t)img.hs.consumed; res->n_chunks = img.n_chunks; res->n_reads = img.reads;
    if (img.n_chunks == 0) return RFQ_OK;
    hipStream_t S = ctx->stream; const int split = a->split_pe ? 1 : 0;
    // bug_compat (split output only): the pieces Repaq::decompressPE decodes, and what it strips and consumes (compat_pieces, dec/ranges.h)
    bool strip1 = (img.hs.last_flags & C_NO_LB) != 0, strip2 = (img.hs.last_flags & C_NO_LB_R2) != 0;
    CompatPlan cp; const bool compat = a->bug_compat != 0 && split;
    if (compat) {
        const int rc = dec_host_table(ctx, img); if (rc) return rc;
        cp = compat_pieces(img.hc.data(), img.n_chunks, true, a->final != 0, img.hs.consumed, C_NO_LB, C_NO_LB_R2);
        strip1 = cp.strip1; strip2 = cp.strip2; res->consumed = (size_t)cp.consumed; res->n_chunks = cp.n_chunks;
    }
    // One pass straight into the caller's buffers (or the context's result buffers); a pass whose text turns out to be >= 4 GiB is redone in ranges,
    // every range into the context's result buffers and from there to its place in the caller's buffers or the context's accumulators.
    const DecDst dst = { { a->d_out1, a->d_out2 }, { a->cap1, a->cap2 } }; DBuf* const acc[2] = { &ctx->out_acc1, &ctx->out_acc2 };
    DecText T; memset(&T, 0, sizeof T); StageSums sums;
    const int rc = dec_each_range(ctx, img, compat ? &cp.pieces : nullptr, sums, "a single chunk decodes to 4 GiB of text or more",
                                  [&](const DecRange& g, const ChunkSpan& r, bool whole) -> int {
        if (whole) return decode_range(ctx, a, g, dst, &T);
        DecText q; const int e = decode_range(ctx, a, g, DecDst{}, &q); if (e) return e;
        for (int k = 0; k < (split ? 2 : 1); k++) {
            const size_t m = q.n[k], w = T.n[k];
            if (!m || (k && r.r1_only)) continue;
            uint8_t* to;
            if (dst.p[k]) { if (w + m > dst.cap[k]) return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffer too small"); to = dst.p[k] + w; }
            else { HIPCHK(ctx, acc[k]->ensure_keep(w + m + 64, w, S)); to = acc[k]->as<uint8_t>() + w; }
            HIPCHK(ctx, hipMemcpyAsync(to, q.p[k], m, hipMemcpyDeviceToDevice, S));
            T.n[k] += m;
        }
        HIPCHK(ctx, hipStreamSynchronize(S));
        T.bases += q.bases; return RFQ_OK;
    });
    if (rc) return rc;
    if (!sums.v.empty()) { for (int k = 0; k < 2; k++) T.p[k] = dst.p[k] ? dst.p[k] : acc[k]->as<uint8_t>(); sums.publish(ctx->timer); }
    res->n_bases = T.bases;
    if (a->final) {   // Repaq::decompress*: drop the final '\n' when the last chunk carries the NO_LINE_BREAK bit
        if (strip1 && T.n[0]) T.n[0]--;
        if (split && strip2 && T.n[1]) T.n[1]--;
    }
    res->d_fq1 = T.p[0]; res->n1 = T.n[0]; res->d_fq2 = split ? T.p[1] : nullptr; res->n2 = split ? T.n[1] : 0;
    return RFQ_OK;
}

// ---- rfq_decode_rows: the reads of an image as fixed-stride base / quality rows.  Always the expanded stage (qdec / sdec in HBM, whatever
// RFQ_MATERIALISE says) with neither text lengths, name middles nor coordinates, then k_dec_rows (dec/rows.h).  Rows of a range start at the
// running read count of the call (DChunk::rbase_abs).
static int rows_range(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const RowsOut& o) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>(); DecStatus* dst = B[DB_STATUS].as<DecStatus>();
    HIPCHK(ctx, hipMemsetAsync(dst, 0, sizeof(DecStatus), S));
    ctx->timer.begin("read_table", S);
    const size_t nr = (size_t)g.n_reads + 2;
    HIPCHK(ctx, B[DB_LEN].ensure(nr * 4)); HIPCHK(ctx, B[DB_OV].ensure(nr * 4));
    DReadTab R; memset(&R, 0, sizeof R); R.len = B[DB_LEN].as<uint32_t>(); R.ov = B[DB_OV].as<int32_t>();
    uint32_t total_bases = 0; U4 pv_tot; memset(&pv_tot, 0, sizeof pv_tot);
    int rc = dec_table_expanded(ctx, a, g, R, false, &total_bases, &pv_tot);
    if (rc) return rc;
    DecExpanded E; rc = dec_streams_expanded(ctx, a, g, R, total_bases, pv_tot, false, &E);
    if (rc) return rc;
    // the streams' verdict before any row is written (the text path refuses the same image here: "corrupt quality buffer")
    DecStatus h; HIPCHK(ctx, ctx->fetch(&h, dst, sizeof h, S)); HIPCHK(ctx, ctx->fetch_sync(S));
    if (h.err & DE_CORRUPT) return rfq_fail(ctx, RFQ_E_FORMAT, "corrupt quality buffer");
    ctx->timer.begin("rows", S);
    // (tiles of 32 reads; no LDS and few registers: eight workgroups per CU)
    const uint32_t bx = grid_x_for(g.n_chunks, (std::max(g.max_reads, 1u) + 31u) / 32u, 8u * ctx->n_cu);
    hipLaunchKernelGGL(k_dec_rows, dim3(bx, g.n_chunks), dim3(256), 0, S, g.CH, (const DevHeader*)D, R, (const uint64_t*)E.qbase, (const uint64_t*)E.sbase,
                       (const uint8_t*)E.qdec, (const uint8_t*)E.sdec, o);
    KCHK(ctx, "k_dec_rows");
    ctx->timer.end(S);
    HIPCHK(ctx, hipStreamSynchronize(S));
    return RFQ_OK;
}

extern "C" int rfq_decode_rows(rfq_ctx* ctx, const rfq_decode_rows_args* ra, rfq_decode_rows_result* res) {
    if (!ctx || !ra || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (ra->n && !ra->d_rfq) return rfq_fail(ctx, RFQ_E_ARG, "null rfq pointer");
    if (ra->base_mode != RFQ_ROWS_ASCII && ra->base_mode != RFQ_ROWS_CODE) return rfq_fail(ctx, RFQ_E_ARG, "base_mode must be RFQ_ROWS_ASCII or RFQ_ROWS_CODE");
    const bool query = !ra->d_bases && !ra->d_quals && !ra->d_lens;
    if (!query && ra->row_len == 0) return rfq_fail(ctx, RFQ_E_ARG, "row_len must be at least 1");
    if ((uintptr_t)ra->d_lens & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens must be 4-byte aligned");
    const rfq_decode_args a = dec_view(ra);
    if (a.n == 0 && a.has_header) return RFQ_OK;                              // an empty .rfq: no reads
    DecImage img; { const int rc = dec_image(ctx, &a, &img); if (rc) return rc; }
    const uint32_t n_chunks = img.n_chunks; const uint64_t n_rows = n_chunks ? img.reads : 0;
    res->consumed = (size_t)img.hs.consumed; res->n_chunks = n_chunks; res->n_rows = n_rows; res->n_bases = n_chunks ? img.bases : 0; res->max_len = n_chunks ? img.hs.max_len : 0;
    if (query || n_chunks == 0) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); ctx->timer.collect(); return RFQ_OK; }
    const uint64_t L = ra->row_len, need = n_rows * L;
    if (L < res->max_len) return rfq_fail(ctx, RFQ_E_NOSPACE, "row_len %u is shorter than the longest read: need row_len >= %u", ra->row_len, res->max_len);
    if (ra->d_bases && ra->bases_cap < need) return rfq_fail(ctx, RFQ_E_NOSPACE, "base rows too small: need %llu bytes (%llu rows of %u)", (unsigned long long)need,
            (unsigned long long)n_rows, ra->row_len);
    if (ra->d_quals && ra->quals_cap < need) return rfq_fail(ctx, RFQ_E_NOSPACE, "quality rows too small: need %llu bytes (%llu rows of %u)", (unsigned long long)need,
            (unsigned long long)n_rows, ra->row_len);
    if (ra->d_lens && ra->lens_cap < n_rows) return rfq_fail(ctx, RFQ_E_NOSPACE, "length array too small: need %llu entries", (unsigned long long)n_rows);
    RowsOut o; memset(&o, 0, sizeof o);
    o.bases = ra->d_bases; o.quals = ra->d_quals; o.lens = ra->d_lens; o.row_len = L; o.n_rows = n_rows;
    o.codes = ra->base_mode == RFQ_ROWS_CODE ? 1u : 0u;
    o.qoff4 = ra->qual_offset * 0x01010101u; o.pad_b4 = ra->pad_base * 0x01010101u; o.pad_q4 = ra->pad_qual * 0x01010101u;
    o.vec = rows_vec(L, ra->d_bases, ra->d_quals);
    // the text path's ranges: bases and qualities of a pass are placed by 32-bit prefix sums
    StageSums sums;
    const int rc = dec_each_range(ctx, img, nullptr, sums, "a single chunk holds 4 Gi bases or 2 Gi reads or more",
                                  [&](const DecRange& g, const ChunkSpan&, bool) -> int { return g.bases >= RANGE_MAX_BASES ? RFQ_RANGE_TOO_BIG : rows_range(ctx, &a, g, o); });
    if (rc) return rc;
    dec_timings(ctx, sums);
    return RFQ_OK;
}

// ---- rfq_decode_names: the name lines of an image back to back and their offsets - what rfq_rows_in takes beside the rows of rfq_decode_rows.  The walk, then
// per range (the ranges of rfq_decode_rows) the coordinate decoder, the lengths kernel, one 64-bit scan over the chunks' totals and the writer (dec/names.h):
// neither the read table nor the expanded stage, a name needs none of the base / quality streams.  The sizes of every range are known before a byte is
// written (a cap that is too small writes nothing); an image of several ranges runs the lengths of each range twice, its buffers are the next range's.
// Workspace: the chunk-local name prefixes live in B[DB_PQL], the per-read piece prefixes in B[DB_PVL], the chunks' totals / bases in B[DB_CTEXT] / B[DB_TBASE].
struct NamesSize { uint64_t bytes; uint32_t max_name; };
static int names_lengths(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, NamesSize* z) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; const DevHeader* D = ctx->d_hdr.as<DevHeader>(); DecStatus* dst = B[DB_STATUS].as<DecStatus>();
    HIPCHK(ctx, hipMemsetAsync(dst, 0, sizeof(DecStatus), S));
    ctx->timer.begin("name_lens", S);
    const size_t nr = (size_t)g.n_reads + 2, nc = (size_t)g.n_chunks + 2;
    HIPCHK(ctx, B[DB_XV].ensure(nr * 4)); HIPCHK(ctx, B[DB_YV].ensure(nr * 4)); HIPCHK(ctx, B[DB_PQL].ensure((nr + nc) * 4));
    if (g.per_read_pieces) HIPCHK(ctx, B[DB_PVL].ensure((nr + nc) * 8));
    HIPCHK(ctx, B[DB_CTEXT].ensure(nc * 8)); HIPCHK(ctx, B[DB_TBASE].ensure(nc * 8)); HIPCHK(ctx, B[DB_SCAN].ensure((nc / SCAN_TILE + 2) * 16 + 1024));
    hipLaunchKernelGGL(k_dec_coords, dim3(2, g.n_chunks), dim3(64), 0, S, a->d_rfq, g.CH, D, B[DB_XV].as<uint32_t>(), B[DB_YV].as<uint32_t>());
    KCHK(ctx, "k_dec_coords");
    hipLaunchKernelGGL(k_dec_namelen, dim3(g.n_chunks), dim3(256), 0, S, a->d_rfq, g.CH, D, (const uint32_t*)B[DB_XV].as<uint32_t>(), (const uint32_t*)B[DB_YV].as<uint32_t>(),
                       B[DB_PQL].as<uint32_t>(), g.per_read_pieces ? B[DB_PVL].as<uint2>() : (uint2*)nullptr, B[DB_CTEXT].as<unsigned long long>(), dst);
    KCHK(ctx, "k_dec_namelen");
    scan_exclusive<unsigned long long>(S, B[DB_CTEXT].as<unsigned long long>(), B[DB_TBASE].as<unsigned long long>(), g.n_chunks, B[DB_SCAN].as<unsigned long long>(), 1);
    ctx->timer.end(S);
    unsigned long long total = 0; DecStatus h;
    HIPCHK(ctx, ctx->fetch(&total, B[DB_TBASE].as<unsigned long long>() + g.n_chunks, 8, S));
    HIPCHK(ctx, ctx->fetch(&h, dst, sizeof h, S)); HIPCHK(ctx, ctx->fetch_sync(S));
    // (k_dec_namelen: list_need = the largest chunk's name bytes, max_one = the longest name; a chunk's prefixes are 32-bit)
    if (h.list_need >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "a single chunk holds 4 GiB of names or more");
    z->bytes = total; z->max_name = h.max_one;
    return RFQ_OK;
}
// the writer of a range whose lengths are in place (names_lengths right before it)
static int names_write(rfq_ctx* ctx, const rfq_decode_args* a, const DecRange& g, const NamesOut& o) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    ctx->timer.begin("names", S);
    // (27 KB of LDS: five workgroups per CU)
    const uint32_t bx = grid_x_for(g.n_chunks, (std::max(g.max_reads, 1u) + NM_READS - 1u) / NM_READS, 5u * ctx->n_cu);
    hipLaunchKernelGGL(k_dec_names, dim3(bx, g.n_chunks), dim3(256), 0, S, a->d_rfq, (uint64_t)a->n, g.CH, ctx->d_hdr.as<DevHeader>(),
                       (const uint32_t*)B[DB_XV].as<uint32_t>(), (const uint32_t*)B[DB_YV].as<uint32_t>(), (const uint32_t*)B[DB_PQL].as<uint32_t>(),
                       g.per_read_pieces ? (const uint2*)B[DB_PVL].as<uint2>() : (const uint2*)nullptr, (const unsigned long long*)B[DB_TBASE].as<unsigned long long>(), o, g.n_chunks);
    KCHK(ctx, "k_dec_names");
    ctx->timer.end(S);
    HIPCHK(ctx, hipStreamSynchronize(S));
    return RFQ_OK;
}

extern "C" int rfq_decode_names(rfq_ctx* ctx, const rfq_decode_names_args* na, rfq_decode_names_result* res) {
    if (!ctx || !na || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (na->n && !na->d_rfq) return rfq_fail(ctx, RFQ_E_ARG, "null rfq pointer");
    if ((uintptr_t)na->d_name_off & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_name_off must be 8-byte aligned");
    const bool query = na->size_only != 0;
    const rfq_decode_args a = dec_view(na);
    DecImage img; { const int rc = dec_image(ctx, &a, &img); if (rc) return rc; }      // (an empty .rfq: no reads, offsets { 0 })
    hipStream_t S = ctx->stream;
    const uint32_t n_chunks = img.n_chunks; const uint64_t n_rows = n_chunks ? img.reads : 0;
    res->consumed = (size_t)img.hs.consumed; res->n_chunks = n_chunks; res->n_rows = n_rows;
    // (the offsets' size is known here: a caller's array that cannot hold them is refused before any length is looked at)
    if (!query && na->d_name_off && na->off_cap < n_rows + 1) return rfq_fail(ctx, RFQ_E_NOSPACE, "offset array too small: need %llu entries", (unsigned long long)(n_rows + 1));
    // the ranges of rfq_decode_rows (the reads of a range count from 0 in 32 bits), twice: every range's bytes - 64-bit from here on: range bases are
    // sums on the host, chunk bases a 64-bit scan -, then the writer
    StageSums sums; const char* const too_big = "a single chunk holds 2 Gi reads or more";
    uint64_t names_len = 0; uint32_t max_name = 0;
    int rc = dec_each_range(ctx, img, nullptr, sums, too_big, [&](const DecRange& g, const ChunkSpan&, bool) -> int {
        NamesSize z; const int e = names_lengths(ctx, &a, g, &z); if (e) return e;
        names_len += z.bytes; max_name = std::max(max_name, z.max_name);
        return RFQ_OK;
    });
    if (rc) return rc;
    res->names_len = names_len; res->max_name = max_name;
    if (query) { HIPCHK(ctx, hipStreamSynchronize(S)); dec_timings(ctx, sums); return RFQ_OK; }
    if (na->d_names && na->names_cap < names_len) return rfq_fail(ctx, RFQ_E_NOSPACE, "name blob too small: need %llu bytes", (unsigned long long)names_len);
    NamesOut o; memset(&o, 0, sizeof o);
    if (na->d_names) o.names = na->d_names; else { HIPCHK(ctx, ctx->names_blob.ensure((size_t)names_len + 64)); o.names = ctx->names_blob.as<uint8_t>(); }
    if (na->d_name_off) o.off = na->d_name_off; else { HIPCHK(ctx, ctx->names_off.ensure((size_t)(n_rows + 1) * 8)); o.off = ctx->names_off.as<uint64_t>(); }
    o.end = names_len;
    if (!n_chunks) { HIPCHK(ctx, hipMemsetAsync(o.off, 0, 8, S)); HIPCHK(ctx, hipStreamSynchronize(S)); }
    // (one pass: the lengths of the sizes pass are still in place; a range's are gone, its buffers were the next range's: once more)
    rc = dec_each_range(ctx, img, nullptr, sums, too_big, [&](const DecRange& g, const ChunkSpan&, bool whole) -> int {
        NamesSize z = { 0, 0 };
        if (!whole) { const int e = names_lengths(ctx, &a, g, &z); if (e) return e; }
        const int e = names_write(ctx, &a, g, o); if (e) return e;
        o.base += z.bytes;
        return RFQ_OK;
    });
    if (rc) return rc;
    dec_timings(ctx, sums);
    res->d_names = o.names; res->d_name_off = o.off;
    return RFQ_OK;
}
