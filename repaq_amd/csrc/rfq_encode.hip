// rfq_encode.hip — host orchestration of the gfx950 FASTQ -> RFQ path (rfq_encode_batch of include/rfq_hip.h).
// Replaces, per batch: Repaq::compress / compressPE chunking (src/repaq.cpp:530-762), RfqCodec::makeHeader
// (src/rfqcodec.cpp:20-145), RfqCodec::encodeChunk (:147-586) and RfqChunk::write (src/rfqchunk.cpp:230-311).
#include "rfq_ctx.h"
#include <type_traits>
#include "rfq_encode_kernels.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <cstddef>

enum EncBuf {   // indices into rfq_ctx::b
    B_BITMAP0 = 0, B_BITMAP1, B_BLK0, B_BLK1, B_LO0, B_LO1, B_SCANTMP,
    B_LEN, B_N1LEN, B_N2OFF, B_X, B_Y, B_TILE, B_LANE, B_OK, B_CHUNK, B_STORED, B_EQ2, B_PQ, B_PV, B_PVIN,
    B_ULEN, B_P, B_MINMAX, B_FIRST, B_CFLAGS, B_IL, B_HIST, B_NCOUNT, B_SCAP, B_SOFF, B_SSIZE, B_XSIZE, B_YSIZE, B_QBASE, B_SBASE,
    B_IMGSIZE, B_IMGOFF, B_CTOTAL, B_CBASE, B_LAYOUT, B_HSTATS, B_OVB, B_OVRAW, B_QCAT, B_SCAT, B_SCRATCH, B_XS, B_YS, B_SEGB, B_SEGC,
    B_NORM0, B_NORM1, B_OT0, B_OT1, B_ONX0, B_ONX1, B_TBITS, B_SBITS, B_NKEEP, B_NTERM, B_NMAP, B_ADJ, B_PINFO, B_SEGM, B_LPK, B_LNB, B_SPK, B_SNM, B_RFLAG, B_SCANTMP2, B_CTOTALN, B_CBASEN, B_SCRATCHN, B_PTOT, B_QPLANE, B_SEGD, B_SEGS, B_SD, B_RN, B_ENC_END
};

static_assert(B_ENC_END <= 80, "encode buffers must stay below the decode buffer indices of rfq_ctx::b");

static int fetch_bytes(rfq_ctx* ctx, const uint8_t* d, size_t n, std::string& out) {
    out.resize(n);
    if (n) HIPCHK(ctx, hipMemcpy(&out[0], d, n, hipMemcpyDeviceToHost));
    return RFQ_OK;
}
// text of line k of read g (host copy), for the reference's error messages
static int fetch_line(rfq_ctx* ctx, const Text& T, uint32_t g, int k, std::string& out) {
    int s = 0; uint32_t r = g; if (T.paired == 1) { s = (int)(g & 1u); r = g >> 1; }
    uint32_t lo2[2];
    HIPCHK(ctx, hipMemcpy(lo2, T.lo[s] + 4 * (size_t)r + k, 8, hipMemcpyDeviceToHost));
    return fetch_bytes(ctx, T.fq[s] + lo2[0], lo2[1] - 1 - lo2[0], out);
}

// RfqHeader::read (src/rfqheader.cpp:19-43) + the derived tables, on device and mirrored on the host
int rfq_upload_header(rfq_ctx* c, const uint8_t* h, size_t n) {
    if (n < 17) return rfq_fail(c, RFQ_E_FORMAT, "Not a valid repaq file!");
    if (h[8] != 2) return rfq_fail(c, RFQ_E_FORMAT, "The data is encoded by different version of repaq, please try repaq v%.5s. \nSee: https://github.com/OpenGene/repaq/releases", (const char*)h + 3);
    const size_t len = 17u + h[16];
    if (n < len) return rfq_fail(c, RFQ_E_FORMAT, "Not a valid repaq file!");
    if (h[0] != 'R' || h[1] != 'F' || h[2] != 'Q') return rfq_fail(c, RFQ_E_FORMAT, "Not a valid repaq file!");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->d_hdr.ensure(sizeof(DevHeader)));
    // The derived tables (hdr_derive: the same function the header kernels call) are made HERE, on the host, and the whole DevHeader goes to the device in one
    // stream-ordered copy from a page-locked block: no kernel, no read-back, no wait (round 5: upload, k_hdr_from_bytes, fetch, synchronise - two round trips in
    // front of every decode that starts with a header).  Bytes equal to the header the device already holds: nothing is sent.
    DevHeader tmp; memset(&tmp, 0, sizeof tmp); memcpy(tmp.bytes, h, len); hdr_derive(&tmp);
    const bool same = c->have_hdr && c->hdr_on_device && c->h_hdr.len == tmp.len && !memcmp(c->h_hdr.bytes, tmp.bytes, tmp.len);
    if (!same) {
        if (!c->pin_up) { if (hipHostMalloc((void**)&c->pin_up, sizeof(DevHeader), 0) != hipSuccess) { c->pin_up = nullptr; (void)hipGetLastError(); } }
        if (c->pin_up) {
            if (c->ev_up_pending) { HIPCHK(c, hipEventSynchronize(c->ev_up)); c->ev_up_pending = false; }       // (the block's previous copy)
            if (!c->ev_up) HIPCHK(c, hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
            memcpy(c->pin_up, &tmp, sizeof tmp);
            HIPCHK(c, hipMemcpyAsync(c->d_hdr.p, c->pin_up, sizeof tmp, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipEventRecord(c->ev_up, c->stream)); c->ev_up_pending = true;
        } else { HIPCHK(c, hipMemcpyAsync(c->d_hdr.p, &tmp, sizeof tmp, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
        c->h_hdr = tmp; c->hdr_on_device = true;
    }
    c->have_hdr = true; c->new_file();   // (another file: what its name pieces fit / whether its reads have one length is not known yet)
    return RFQ_OK;
}

// Mapping of a normalised stream (see k_norm_classify) back to the caller's text
struct NormMap { const uint32_t* ot[2]; const uint32_t* onx[2]; size_t orig_n[2]; };
#define RFQ_NEED_NORM 1            // internal: the '\n'-only indexer met '\r' or an empty line; redo on normalised text
#define RFQ_RETRY_ROOM 3           // internal: an arena sized in advance was too small (it has been grown): encode the batch again

// FastqReader::getLine semantics for text with '\r' / blank lines: rewrite stream s as '\n'-terminated text + the line maps
static int normalize_stream(rfq_ctx* ctx, const uint8_t* fq, size_t n, uint64_t file_off, bool final, int s, NormMap& nm, const uint8_t** out, size_t* out_n) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    nm.orig_n[s] = n; nm.ot[s] = nm.onx[s] = nullptr; *out = nullptr; *out_n = 0;
    if (n == 0) return RFQ_OK;
    const uint64_t nwords = (n + 63) / 64; const uint32_t nblk = (uint32_t)((nwords + 255) / 256);
    HIPCHK(ctx, B[B_TBITS].ensure(nwords * 8 + 64)); HIPCHK(ctx, B[B_SBITS].ensure(nwords * 8 + 64));
    HIPCHK(ctx, B[B_NKEEP].ensure(((size_t)nblk + 2) * 4)); HIPCHK(ctx, B[B_NTERM].ensure(((size_t)nblk + 2) * 4));
    HIPCHK(ctx, B[B_SCANTMP].ensure(std::max<size_t>(1024, ((size_t)nblk / SCAN_TILE + 2) * 16)));
    NormIn in; in.fq = fq; in.n = (uint32_t)n; in.file_off = file_off; in.file_end = final ? file_off + n : ~0ull;
    hipLaunchKernelGGL(k_norm_classify, dim3(nblk), dim3(256), 0, S, in, B[B_TBITS].as<uint64_t>(), B[B_SBITS].as<uint64_t>(), B[B_NKEEP].as<uint32_t>(),
            B[B_NTERM].as<uint32_t>());
    KCHK(ctx, "k_norm_classify");
    scan_exclusive<uint32_t>(S, B[B_NKEEP].as<uint32_t>(), B[B_NKEEP].as<uint32_t>(), nblk, B[B_SCANTMP].as<uint32_t>(), 1);
    scan_exclusive<uint32_t>(S, B[B_NTERM].as<uint32_t>(), B[B_NTERM].as<uint32_t>(), nblk, B[B_SCANTMP].as<uint32_t>(), 1);
    uint32_t keep = 0, terms = 0;
    HIPCHK(ctx, ctx->fetch(&keep, B[B_NKEEP].as<uint32_t>() + nblk, 4, S));
    HIPCHK(ctx, ctx->fetch(&terms, B[B_NTERM].as<uint32_t>() + nblk, 4, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    HIPCHK(ctx, B[B_NORM0 + s].ensure((size_t)keep + 64)); HIPCHK(ctx, B[B_OT0 + s].ensure(((size_t)terms + 4) * 4));
            HIPCHK(ctx, B[B_ONX0 + s].ensure(((size_t)terms + 4) * 4));
    hipLaunchKernelGGL(k_norm_emit, dim3(nblk), dim3(256), 0, S, in, (const uint64_t*)B[B_TBITS].as<uint64_t>(), (const uint64_t*)B[B_SBITS].as<uint64_t>(),
                       (const uint32_t*)B[B_NKEEP].as<uint32_t>(), (const uint32_t*)B[B_NTERM].as<uint32_t>(), B[B_NORM0 + s].as<uint8_t>(), B[B_OT0 + s].as<uint32_t>(), B[B_ONX0 + s].as<uint32_t>());
    hipLaunchKernelGGL(k_norm_tail, dim3(1), dim3(64), 0, S, B[B_OT0 + s].as<uint32_t>(), B[B_ONX0 + s].as<uint32_t>(), terms, (uint32_t)n);
    KCHK(ctx, "k_norm_emit");
    nm.ot[s] = B[B_OT0 + s].as<uint32_t>(); nm.onx[s] = B[B_ONX0 + s].as<uint32_t>();
    *out = B[B_NORM0 + s].as<uint8_t>(); *out_n = keep;
    return RFQ_OK;
}
// ---------------------------------------------------------------- one attempt at one text: the batch as values, its stages, encode_impl
#define RFQ_AGAIN_LAZY 2           // internal: the index without a read-back could not take this batch (ctx->lazy_block is up): the attempt once more
#define RFQ_AGAIN_ENDED 4          // internal: the reader stops at an empty line: the attempt once more, the input ended there (EncAgain)
#define RFQ_AGAIN_MIRROR 5         // internal: stream 1 could not be read through stream 0's line table after all: the attempt once more with an index per stream (encode_impl)
struct EncAgain { uint32_t unit_cap = ~0u; bool ended = false; };   // what a repeat of the attempt starts from: the call's own arguments, or the unit the reader stopped at
// The call as one attempt sees it (the head of encode_impl).  hs, the host copy of the status block, is also what the upload of a fresh block reads: it lives as long as the attempt.
struct EncBatch {
    const rfq_encode_args* a; const NormMap* nm; const uint32_t* skip; bool scan_only, ended, fin, is_pe;
    // mirror_ok: the caller has a gather behind the index and may be given stream 0's line table for both streams; mirrored: enc_index did so; mirror_proven: the
    // final read-back says that stream 1's line ends are where stream 0's are
    bool mirror_ok, mirrored, mirror_proven; uint32_t unit_cap; int nstreams; const uint8_t* fq[2]; size_t nbytes[2]; Text T; DevStatus* dst; DevStatus hs;
    uint64_t orig_n(int s) const { return nm ? nm->orig_n[s] : nbytes[s]; }
};
// what index + cut produced (enc_index: lazy, guess_units, nlines, nrec; enc_cut: the rest, the maxima from the partition's read-back).  n_chunks == 0: nothing to encode
struct EncCut {
    bool lazy; uint32_t guess_units, nlines[2], nrec[2], n_units, n_reads, n_chunks, cap_chunks, units_used, reads_used, max_reads, max_rec, max_len, max_chunk_bases; uint64_t total_bases;
};
// the device tables that more than one stage reads, each pointer taken where its buffer is ensured (enc_cut: R, C.first, scantmp; enc_tables; the stage that fills it)
struct EncTables {
    ReadTab R; ChunkTab C; Layout* L; DevHeader* D; int8_t* ovb; int16_t* ovraw; uint32_t *cbits, *cfail, *redo; void* scantmp;
    size_t nr, nc, nsb, catbytes; uint32_t n_seg; uint32_t *segb, *segm; int* segc; uint64_t *ctot, *cbase, *ctot_n, *cbase_n;
    uint8_t* qcat; uint32_t* spk; uint16_t* snm; uint32_t* qplane; uint8_t *scratch, *scratch_n, *xs, *ys, *img; uint64_t img_cap, hdr_bytes;
};
// which formulation runs (enc_form; enc_header: make_header, hdr_aside; enc_gather_tiles: aux_chain, coder_waits)
struct EncForm { bool fast; uint32_t kshift; bool make_header, hdr_aside, masks, coder_list; uint32_t nqg; bool aux_chain, coder_waits; };
// (an early return must not leave the second stream running over buffers that are about to be reused - by the caller, or by the repeat of the attempt, which
// rebuilds nothing but starts its own search over the same buffers)
struct AuxGuard { rfq_ctx* c; bool armed; ~AuxGuard() { if (armed) (void)hipStreamSynchronize(c->aux); } };
// a buffer of the context sized for this batch and its typed pointer, in one step
template <class T> static hipError_t table(DBuf& d, size_t bytes, T*& p) { const hipError_t e = d.ensure(bytes); p = (T*)d.p; return e; }
static int empty_result(rfq_ctx* ctx, rfq_encode_result* res) { ctx->chunk_off.assign(1, 0); res->h_chunk_off = ctx->chunk_off.data(); return RFQ_OK; }
static hipError_t fresh_status(rfq_ctx* ctx, EncBatch& b) {               // a clean status block, on the host and (stream-ordered) on the device
    memset(&b.hs, 0, sizeof b.hs); b.hs.err_key = ~0ull; b.hs.coord_key = ~0ull; b.hs.first_empty = ~0u;
    return hipMemcpyAsync(b.dst, &b.hs, sizeof b.hs, hipMemcpyHostToDevice, ctx->stream);
}
// an offset in the indexed text -> the caller's stream: not past its end (a virtual terminator past an unterminated last line), counted from the stream's own first byte
static uint64_t consumed_of(const EncBatch& b, int s, uint64_t v) { const uint64_t lim = b.orig_n(s); if (v > lim) v = lim; return b.nm ? v : v - b.skip[s]; }

// ---- phase 1: the line index lo[] of every stream.  One pass (k_line_index) where the lines are long enough for a table sized in advance
// (RFQ_INDEX=2pass, or more than one line per 16 bytes: newline bitmap -> scan -> k_line_offsets, the table sized exactly)
static int enc_index(rfq_ctx* ctx, EncBatch& b, EncCut& cut) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    ctx->timer.begin("index", S);
    uint32_t nblk[2] = { 0, 0 }; uint64_t nwords[2] = { 0, 0 };
    for (int s = 0; s < b.nstreams; s++) { nwords[s] = (b.nbytes[s] + 63) / 64; nblk[s] = (uint32_t)((nwords[s] + 255) / 256); }
    int idx_tiles = ctx->opt.idx_tiles ? ctx->opt.idx_tiles : NLF_TILES;
    if (idx_tiles != 4 && idx_tiles != 8 && idx_tiles != 16) idx_tiles = NLF_TILES;
    uint32_t nidx[2] = { 0, 0 };                                                           // workgroups of the one-pass index
    for (int s = 0; s < b.nstreams; s++) nidx[s] = (uint32_t)((b.nbytes[s] + idx_tiles * 16384u - 1) / (idx_tiles * 16384u));
    uint32_t n_newlines[2] = { 0, 0 }; uint8_t lastbyte[2] = { '\n', '\n' };
    bool one_pass = !ctx->opt.index_2pass;
    // MIRROR: the mates of untrimmed sequencer output differ in one digit of their names - two texts of one size with their line ends at the same offsets.  Stream 1 is
    // not indexed then: it is read through stream 0's table (every offset in it is < n[0] == n[1]: nothing reads outside stream 1), k_gather2 proves as it goes that each
    // record it stages has its four line feeds where the table says and no '\r', k_mirror_tail does the same for the text behind the last encoded unit, and the verdict
    // comes back with the batch's own read-backs.  Where it does not hold the attempt is thrown away and repeated with both indexes (encode_impl; ctx->mirror_block).
    const bool mirror = b.mirrored = b.mirror_ok && one_pass && b.nstreams == 2 && !b.nm && !ctx->opt.no_mirror && !ctx->mirror_block && nblk[0] != 0 &&
                                     b.nbytes[0] == b.nbytes[1] && b.skip[0] == b.skip[1];
    // LAZY: no read-back behind the index.  The per-read tables are sized for a unit count guessed from the records per byte of the context's earlier batches; the
    // index's totals stay on the device (k_index_totals: lines, units, the unterminated tail) and reach the host with the partition's results.  A batch that holds
    // more units than guessed, an index that has to fall back to two passes: once more with the read-back (ctx->lazy_block).
    const bool lazy_allowed = !ctx->lazy_block; ctx->lazy_block = false;
    bool lazy = one_pass && lazy_allowed && ctx->rec_per_byte > 0.0 && !ctx->mixed_lengths && b.unit_cap == ~0u && !b.ended;
    uint32_t guess_units = 0;
    if (lazy) {
        double g = 1e300;
        for (int s = 0; s < b.nstreams; s++) g = std::min(g, (double)b.nbytes[s] * ctx->rec_per_byte * 1.03 + 64.0);
        if (b.a->paired == RFQ_PE_INTERLEAVED) g *= 0.5;
        if (g > 2.0e9 || g < 1.0) lazy = false; else guess_units = (uint32_t)g;
        for (int s = 0; s < b.nstreams; s++) if (!nblk[s]) lazy = false;
    }
    if (one_pass) {
        size_t cap[2] = { 0, 0 };
        for (int s = 0; s < b.nstreams; s++) {
            if (!nblk[s]) continue;
            if (mirror && s == 1) { if (!lazy) HIPCHK(ctx, ctx->fetch(&lastbyte[1], b.fq[1] + b.nbytes[1] - 1, 1, S)); continue; }   // (its own last byte, nothing else)
            cap[s] = std::max(B[B_LO0 + s].cap / 4, b.nbytes[s] / 16 + 4096);
            HIPCHK(ctx, B[B_LO0 + s].ensure(cap[s] * 4));
            HIPCHK(ctx, B[B_BLK0 + s].ensure((size_t)nidx[s] * 8 + 64));                  // state words, then the ticket and the total
            HIPCHK(ctx, hipMemsetAsync(B[B_BLK0 + s].p, 0, (size_t)nidx[s] * 8 + 64, S));
            unsigned long long* state = B[B_BLK0 + s].as<unsigned long long>();
            uint32_t* tt = (uint32_t*)(state + nidx[s]);
            const uint32_t lo_cap = (uint32_t)std::min<size_t>(cap[s] - 4, 0xFFFFFFF0u);
            auto kern = idx_tiles == 16 ? k_line_index<16> : (idx_tiles == 4 ? k_line_index<4> : k_line_index<8>);
            hipLaunchKernelGGL(kern, dim3(nidx[s]), dim3(256), 0, S, b.fq[s], (uint32_t)b.nbytes[s], b.skip[s], B[B_LO0 + s].as<uint32_t>(), lo_cap, state, tt, tt + 1, b.dst);
            KCHK(ctx, "k_line_index");
            if (lazy) continue;
            HIPCHK(ctx, ctx->fetch(&n_newlines[s], tt + 1, 4, S));
            HIPCHK(ctx, ctx->fetch(&lastbyte[s], b.fq[s] + b.nbytes[s] - 1, 1, S));
        }
        if (lazy) {
            const uint32_t* t0 = (const uint32_t*)(B[B_BLK0].as<unsigned long long>() + nidx[0]) + 1;
            const uint32_t* t1 = b.nstreams == 2 && !mirror ? (const uint32_t*)(B[B_BLK1].as<unsigned long long>() + nidx[1]) + 1 : t0;
            hipLaunchKernelGGL(k_index_totals, dim3(1), dim3(64), 0, S, t0, t1, b.fq[0], (uint32_t)b.nbytes[0], b.fq[1], (uint32_t)b.nbytes[1], B[B_LO0].as<uint32_t>(),
                               b.nstreams == 2 ? B[mirror ? B_LO0 : B_LO1].as<uint32_t>() : (uint32_t*)nullptr, b.a->final ? 1 : 0, (int)b.a->paired, b.unit_cap, guess_units, b.dst,
                               mirror ? 1 : 0);
            KCHK(ctx, "k_index_totals");
        } else {
            HIPCHK(ctx, ctx->fetch(&b.hs, b.dst, sizeof b.hs, S));
            HIPCHK(ctx, ctx->fetch_sync(S));
            if (mirror) {
                // stream 0's totals for both; a table that needs the two-pass index, a last byte that ends a line in one stream only: not this way
                n_newlines[1] = n_newlines[0];
                if ((b.hs.err & DE_INDEX_RETRY) || (lastbyte[0] != '\n') != (lastbyte[1] != '\n')) return RFQ_AGAIN_MIRROR;
            }
        }
        if (!lazy && (b.hs.err & DE_INDEX_RETRY)) {                                                    // start over with a clean status block
            one_pass = false;
            HIPCHK(ctx, fresh_status(ctx, b));
            HIPCHK(ctx, hipStreamSynchronize(S));                                         // (hs is a host object the copy reads, and the next read-back writes it)
            n_newlines[0] = n_newlines[1] = 0;
        }
    }
    if (!one_pass) {
        ctx->timer.end(S); ctx->timer.begin("index_2pass", S);
        size_t scantmp = 1024;
        for (int s = 0; s < b.nstreams; s++) {
            HIPCHK(ctx, B[B_BITMAP0 + s].ensure(nwords[s] * 8 + 64));
            HIPCHK(ctx, B[B_BLK0 + s].ensure(((size_t)nblk[s] + 2) * 4));
            scantmp = std::max(scantmp, ((size_t)nblk[s] / SCAN_TILE + 2) * 16);
        }
        HIPCHK(ctx, B[B_SCANTMP].ensure(scantmp));
        for (int s = 0; s < b.nstreams; s++) {
            if (!nblk[s]) continue;
            hipLaunchKernelGGL(k_nl_bitmap, dim3(nblk[s]), dim3(256), 0, S, b.fq[s], (uint32_t)b.nbytes[s], b.skip[s], B[B_BITMAP0 + s].as<uint64_t>(),
                    B[B_BLK0 + s].as<uint32_t>(), b.dst);
            KCHK(ctx, "k_nl_bitmap");
            scan_exclusive<uint32_t>(S, B[B_BLK0 + s].as<uint32_t>(), B[B_BLK0 + s].as<uint32_t>(), nblk[s], B[B_SCANTMP].as<uint32_t>(), 1);
        }
        for (int s = 0; s < b.nstreams; s++) {
            if (!nblk[s]) continue;
            HIPCHK(ctx, ctx->fetch(&n_newlines[s], B[B_BLK0 + s].as<uint32_t>() + nblk[s], 4, S));
            HIPCHK(ctx, ctx->fetch(&lastbyte[s], b.fq[s] + b.nbytes[s] - 1, 1, S));
        }
        HIPCHK(ctx, ctx->fetch(&b.hs, b.dst, sizeof b.hs, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
    }
    if (!lazy && (b.hs.err & DE_HAS_CR)) return b.nm ? rfq_fail(ctx, RFQ_E_HIP, "internal: '\\r' in normalised text") : RFQ_NEED_NORM;
    cut.nlines[0] = cut.nlines[1] = cut.nrec[0] = cut.nrec[1] = 0;
    for (int s = 0; s < b.nstreams && !lazy; s++) {
        // an unterminated tail is the file's last line only in the final batch; in a non-final batch it is a line cut by the
        // batch boundary and belongs to the next batch
        const int unterm = b.a->final && b.nbytes[s] > 0 && lastbyte[s] != '\n';
        cut.nlines[s] = n_newlines[s] + (unterm ? 1u : 0u); cut.nrec[s] = cut.nlines[s] / 4;
        if (mirror && s == 1) continue;                                     // (stream 0's table, virtual terminator included)
        if (!one_pass || !nblk[s]) HIPCHK(ctx, B[B_LO0 + s].ensure(((size_t)cut.nlines[s] + 4) * 4));
        if (nblk[s]) {
            if (!one_pass) hipLaunchKernelGGL(k_line_offsets, dim3(nblk[s]), dim3(256), 0, S, B[B_BITMAP0 + s].as<uint64_t>(), B[B_BLK0 + s].as<uint32_t>(),
                    (uint32_t)b.nbytes[s], b.skip[s], B[B_LO0 + s].as<uint32_t>());
            hipLaunchKernelGGL(k_line_tail, dim3(1), dim3(64), 0, S, B[B_LO0 + s].as<uint32_t>(), n_newlines[s], (uint32_t)b.nbytes[s], unterm);
            KCHK(ctx, "k_line_offsets");
        }
    }
    ctx->timer.end(S);
    // (a marker, not a phase: the index's totals stay on the device until the partition's read-back - tests look for it)
    if (lazy) { ctx->timer.begin("lazy_index", S); ctx->timer.end(S); }
    if (mirror) { ctx->timer.begin("mirror_index", S); ctx->timer.end(S); }     // (the same: one line index served both streams)
    cut.lazy = lazy; cut.guess_units = guess_units;
    Text& T = b.T; memset(&T, 0, sizeof T);
    for (int s = 0; s < 2; s++) { T.fq[s] = b.fq[s]; T.n[s] = (uint32_t)b.nbytes[s]; T.lo[s] = s < b.nstreams ? B[mirror ? B_LO0 : B_LO0 + s].as<uint32_t>() : nullptr;
            T.ot[s] = b.nm && s < b.nstreams ? b.nm->ot[s] : nullptr; }
    T.paired = b.a->paired; T.upr = b.a->paired == RFQ_SE ? 1u : 2u;
    return RFQ_OK;
}
// ---- phase 2: read table, chunk cuts - up to the partition's read-back and everything the host decides from it
static int enc_cut(rfq_ctx* ctx, EncBatch& b, EncCut& cut, EncTables& t, rfq_encode_result* res, EncAgain* again) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    uint32_t n_units = b.a->paired == RFQ_SE ? cut.nrec[0] : (b.a->paired == RFQ_PE_TWO_FILES ? std::min(cut.nrec[0], cut.nrec[1]) : cut.nrec[0] / 2);
    if (n_units > b.unit_cap) n_units = b.unit_cap;                   // the reader stopped at an empty line (src/fastqreader.cpp:180-191)
    if (cut.lazy) n_units = cut.guess_units;                              // (what the tables are sized for; the true count comes back with the partition)
    uint32_t n_reads = n_units * b.T.upr; b.T.n_reads = n_reads;
    const uint32_t* const nu = cut.lazy ? &b.dst->idx_units : (const uint32_t*)nullptr;      // where the kernels up to the partition find the unit count
    if (n_units == 0) return empty_result(ctx, res);
    ctx->timer.begin("lens+cut", S);
    const size_t nr = t.nr = (size_t)n_reads + 2;
    HIPCHK(ctx, table(B[B_LEN], nr * 4, t.R.len)); HIPCHK(ctx, table(B[B_N1LEN], nr * 4, t.R.name1_len)); HIPCHK(ctx, table(B[B_N2OFF], nr * 4, t.R.name2_off)); HIPCHK(ctx, table(B[B_X], nr * 4, t.R.x));
    HIPCHK(ctx, table(B[B_Y], nr * 4, t.R.y)); HIPCHK(ctx, table(B[B_TILE], nr * 2, t.R.tile)); HIPCHK(ctx, table(B[B_LANE], nr, t.R.lane)); HIPCHK(ctx, table(B[B_OK], nr, t.R.ok)); HIPCHK(ctx, table(B[B_CHUNK], nr * 4, t.R.chunk));
    HIPCHK(ctx, table(B[B_STORED], nr * 4, t.R.stored)); HIPCHK(ctx, table(B[B_EQ2], nr, t.R.eq2)); HIPCHK(ctx, table(B[B_PQ], nr * 4, t.R.pq)); HIPCHK(ctx, table(B[B_PV], nr * 16, t.R.pv)); HIPCHK(ctx, table(B[B_SD], nr * 4, t.R.sd));
    uint64_t *ulen, *P; HIPCHK(ctx, table(B[B_ULEN], ((size_t)n_units + 2) * 8, ulen)); HIPCHK(ctx, table(B[B_P], ((size_t)n_units + 2) * 8, P)); HIPCHK(ctx, B[B_PVIN].ensure(nr * 16));
    HIPCHK(ctx, table(B[B_SCANTMP], std::max<size_t>(1024, (nr / SCAN_TILE + 2) * 16), t.scantmp));
    // sequence lengths come from the line table alone; the names are parsed where the text is staged anyway (k_gather2), or by k_read_table for
    // the reads that need them earlier (chunk 0 of a first batch: the file header) / on the byte-wise gather path (all of them)
    const uint32_t ublocks = (n_units + 255) / 256; uint32_t* minmax; HIPCHK(ctx, table(B[B_MINMAX], ((size_t)ublocks + 2) * LENS_BLK * 4, minmax));
    hipLaunchKernelGGL(k_read_lens, dim3(ublocks), dim3(256), 0, S, b.T, t.R.len, t.R.stored, ulen, n_units, b.T.upr, minmax, b.dst, nu);
    KCHK(ctx, "k_read_lens");
    // every read the same length (sequencer output): both prefixes have a closed form - the scans see the flag and return, k_fill_pq writes g x L (no host round trip)
    uint32_t* const uni = minmax + (size_t)ublocks * LENS_BLK;
    hipLaunchKernelGGL(k_lens_uniform, dim3(1), dim3(1024), 0, S, (const uint32_t*)minmax, ublocks, n_units, uni, nu);
    // The two prefix scans (units for the cut, reads for the base prefix: six launches) see `uni` and return at once when every read has L bases.  A context that has
    // not met reads of several lengths in this file does not even launch them: k_partition says DE_NEED_SCAN if they were needed after all, and scans + partition run
    // then - one more round trip, once per file (ctx->mixed_lengths stays up until the header is cleared).
    auto prefix_scans = [&]() {
        scan_exclusive<uint64_t>(S, ulen, P, n_units, (uint64_t*)t.scantmp, 1, uni);
        scan_exclusive<uint32_t>(S, t.R.len, t.R.pq, n_reads, (uint32_t*)t.scantmp, 1, uni);
    };
    bool have_scans = ctx->mixed_lengths;
    if (have_scans) prefix_scans();
    hipLaunchKernelGGL(k_fill_pq, dim3(n_reads / 256 + 1), dim3(256), 0, S, t.R.pq, n_reads, (const uint32_t*)uni, nu, b.T.upr);
    const uint64_t cap64 = (uint64_t)(b.nbytes[0] + b.nbytes[1]) / (2ull * b.a->chunk_bases) + 3;
    const uint32_t cap_chunks = cut.cap_chunks = (uint32_t)std::min<uint64_t>(cap64, (uint64_t)n_units + 1);
    HIPCHK(ctx, B[B_FIRST].ensure(((size_t)cap_chunks + 2) * 4));
    memset(&t.C, 0, sizeof t.C);
    t.C.first = B[B_FIRST].as<uint32_t>();
    if (b.a->carry_bases && !b.scan_only) return rfq_fail(ctx, RFQ_E_ARG, "carry_bases is for the plan pass (rfq_scan_batch): an encode starts on a chunk boundary");
    if (b.a->carry_bases >= b.a->chunk_bases) return rfq_fail(ctx, RFQ_E_ARG, "carry_bases must be < chunk_bases");
    for (;;) {
        hipLaunchKernelGGL(k_partition, dim3(1), dim3(1024), 0, S, (const uint64_t*)(P + 1), n_units, b.T.upr, b.a->chunk_bases, b.a->carry_bases, b.fin ? 1 : 0,
                           (const uint32_t*)minmax, ublocks, t.C.first, cap_chunks + 1, b.dst, (const uint32_t*)uni, have_scans ? 1 : 0, nu);
        KCHK(ctx, "k_partition");
        HIPCHK(ctx, ctx->fetch(&b.hs, b.dst, sizeof b.hs, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
        if (have_scans || !(b.hs.err & DE_NEED_SCAN)) break;
        ctx->mixed_lengths = true; have_scans = true; prefix_scans();       // (the bit stays in the device's status word: nobody else reads it)
    }
    b.hs.err &= ~(uint32_t)DE_NEED_SCAN;
    ctx->timer.end(S);
    if (b.mirrored && (b.hs.err & DE_MIRROR_FAIL)) return RFQ_AGAIN_MIRROR;     // (k_index_totals: the streams' last bytes)
    if (cut.lazy) {
        // the index's verdict, which the other form reads right behind it
        if (b.hs.err & (DE_INDEX_RETRY | DE_UNITS_GUESS | DE_NEED_SCAN)) { ctx->lazy_block = true; if (b.hs.err & DE_NEED_SCAN) ctx->mixed_lengths = true;
                return RFQ_AGAIN_LAZY; }
        if (b.hs.err & DE_HAS_CR) return b.nm ? rfq_fail(ctx, RFQ_E_HIP, "internal: '\\r' in normalised text") : RFQ_NEED_NORM;
        for (int s = 0; s < b.nstreams; s++) { cut.nlines[s] = b.hs.idx_lines[s]; cut.nrec[s] = cut.nlines[s] / 4; }
        n_units = b.hs.idx_units_true; n_reads = n_units * b.T.upr; b.T.n_reads = n_reads;
        if (n_units == 0) return empty_result(ctx, res);
    }
    { double r = 0.0; for (int s = 0; s < b.nstreams; s++) if (b.nbytes[s]) r = std::max(r, (double)cut.nrec[s] / (double)b.nbytes[s]); if (r > 0.0) ctx->rec_per_byte = r; }
    if (b.hs.err & DE_EMPTY_LINE) {
        // "\n\n" is a swallowed blank line, not an empty one: classify the text properly first.  On normalised text an empty line is
        // where FastqReader::read returns NULL (src/fastqreader.cpp:180-191): the record and everything after it are never read.
        if (!b.nm) return RFQ_NEED_NORM;
        again->unit_cap = b.hs.first_empty / b.T.upr; again->ended = true;
        return RFQ_AGAIN_ENDED;
    }
    if (b.hs.err & DE_INTERNAL) return rfq_fail(ctx, RFQ_E_HIP, "internal: reads of one length, units of several (k_lens_uniform / k_partition disagree)");
    if (b.hs.err & DE_QUAL_SHORT) return rfq_fail(ctx, RFQ_E_UNPINNED, "a quality line is shorter than its sequence line (the reference reads past the string: undefined)");
    cut.n_units = n_units; cut.n_reads = n_reads; cut.n_chunks = b.hs.n_chunks;
    if (cut.n_chunks > cap_chunks) return rfq_fail(ctx, RFQ_E_HIP, "internal: chunk table overflow (%u > %u)", cut.n_chunks, cap_chunks);
    if (cut.n_chunks == 0) return empty_result(ctx, res);
    cut.units_used = b.hs.n_units_used; cut.reads_used = cut.units_used * b.T.upr; cut.total_bases = b.hs.total_bases;
    cut.max_reads = std::max(b.hs.max_chunk_reads, 1u); cut.max_rec = b.hs.max_rec; cut.max_len = b.hs.max_len; cut.max_chunk_bases = b.hs.max_chunk_bases;
    return RFQ_OK;
}
// ---- the plan pass's tail.  rfq_scan_batch stops here: where every chunk ends in the caller's stream(s)
static int enc_chunk_ends(rfq_ctx* ctx, const EncBatch& b, const EncCut& cut, const EncTables& t, rfq_encode_result* res) {
    hipStream_t S = ctx->stream;
    HIPCHK(ctx, ctx->b[B_P].ensure(((size_t)cut.n_chunks + 2) * 16));            // (the unit prefix is no longer needed)
    uint64_t* e1 = ctx->b[B_P].as<uint64_t>(); uint64_t* e2 = e1 + cut.n_chunks + 1;
    hipLaunchKernelGGL(k_chunk_ends, dim3((cut.n_chunks + 255) / 256), dim3(256), 0, S, b.T, (const uint32_t*)t.C.first, cut.n_chunks,
                       b.nm ? b.nm->onx[0] : nullptr, (b.nm && b.nstreams == 2) ? b.nm->onx[1] : nullptr, e1, e2);
    KCHK(ctx, "k_chunk_ends");
    ctx->scan_end[0].assign(cut.n_chunks, 0); ctx->scan_end[1].assign(b.nstreams == 2 ? cut.n_chunks : 0, 0);
    HIPCHK(ctx, ctx->fetch(ctx->scan_end[0].data(), e1, (size_t)cut.n_chunks * 8, S));
    if (b.nstreams == 2) HIPCHK(ctx, ctx->fetch(ctx->scan_end[1].data(), e2, (size_t)cut.n_chunks * 8, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    for (int s = 0; s < 2; s++) for (auto& v : ctx->scan_end[s]) v = consumed_of(b, s, v);
    res->n_chunks = cut.n_chunks; res->n_reads = cut.reads_used; res->n_bases = cut.total_bases; res->reserved = (int32_t)b.hs.unit_bases;
    res->consumed1 = (size_t)ctx->scan_end[0].back(); res->consumed2 = b.nstreams == 2 ? (size_t)ctx->scan_end[1].back() : 0;
    ctx->timer.collect();
    return RFQ_OK;
}
// Which gather (from the cut): the tile gather k_gather2 (+ k_seqpack) whenever two records fit its staged-text buffer - tiles of K reads, the largest power of two
// that always fits - else the byte-wise k_gather (+ k_packbytes).  RFQ_GATHER=old forces the latter (tests run both).  Which coder (header = true: they need the header on
// the host - tile path in front of the gather, byte-wise path behind it, where masks is false by construction).
static void enc_form(const rfq_ctx* ctx, const EncCut& cut, EncForm& f, bool header) {
    const DevHeader& HH = ctx->h_hdr;
    if (!header) { f.kshift = 6; while (f.kshift >= 1 && ((uint64_t)cut.max_rec << f.kshift) + 64u > G2_CAP) f.kshift--; f.fast = f.kshift >= 1 && !ctx->opt.gather_old; return; }
    // match masks for files with at most four coded quality values (a NovaSeq-binned file: ':' ',' '#' and the 0xFF entry the reference's table gets when the
    // N bases have no quality of their own); the most frequent two or three get planes built in LDS, the others are set bit by bit
    f.masks = f.fast && !ctx->opt.qual_bytes && HH.valid && (HH.flags & H_QUAL_BY_COL) && !(HH.flags & H_DONT_QUAL) && HH.n_normal >= 1u && HH.n_normal <= 4u;
    f.nqg = (std::min<uint32_t>(HH.n_normal, NPOS_SLOT) + PC_G - 1) / PC_G;                           // quality-value streams, PC_G per wave
    // the value streams of a file with many coded quality values (no match masks): the list coder - one wave per (chunk, segment) for all of them, work
    // proportional to the coded positions - instead of a wave per four streams testing every position (RFQ_CODER=list / mask force one or the other)
    f.coder_list = !f.masks && !(HH.flags & H_DONT_QUAL) && (HH.flags & H_QUAL_BY_COL) && HH.n_normal >= 1 && (ctx->opt.coder == 1 || (ctx->opt.coder == 0 && HH.n_normal >= 5));
}
// RfqHeader::makeQualityTable's refusals (src/rfqheader.cpp:140-166), as soon as the header kernels' verdict is on the host (tile path: behind the header stage; byte-wise path: behind its gather)
static int header_errors(rfq_ctx* ctx, const EncBatch& b, const EncForm& f) {
    if (b.hs.err & (DE_BAD_QUAL | DE_BAD_BASE)) {
        const uint32_t g = b.hs.err_read, i = (uint32_t)b.hs.err_key; std::string ln;
        if (b.hs.err & DE_BAD_QUAL) { if (fetch_line(ctx, b.T, g, 3, ln)) return RFQ_E_HIP; return rfq_fail(ctx, RFQ_E_DATA, "bad quality value: %d", (int)(int8_t)ln[i]); }
        if (fetch_line(ctx, b.T, g, 1, ln)) return RFQ_E_HIP;
        const char c = ln[i];
        if (c == 'a' || c == 't' || c == 'c') return rfq_fail(ctx, RFQ_E_DATA, "repaq doesn't support FASTQ with lowercase bases (a/t/c/g)\nbut we get:\n%s", ln.c_str());
        return rfq_fail(ctx, RFQ_E_DATA, "repaq only supports FASTQ with uppercase bases (A/T/C/G/N)\nbut we get:\n%s", ln.c_str());
    }
    if (b.hs.err & DE_NO_QUAL_BINS) return rfq_fail(ctx, RFQ_E_DATA, "bad quality string, is this a valid FASTQ file?");
    if (f.make_header) { if (!ctx->h_hdr.valid) return rfq_fail(ctx, RFQ_E_HIP, "internal: header was not finalised"); ctx->have_hdr = true; ctx->hdr_on_device = true; }
    return RFQ_OK;
}
// the per-chunk tables of an encode, and what both gathers leave for the coders: the overlaps, the per-chunk accumulators, the N streams' totals, the position coder's segment tables
static int enc_tables(rfq_ctx* ctx, const EncBatch& b, const EncCut& cut, EncTables& t) {
    DBuf* B = ctx->b; ChunkTab& C = t.C; const size_t nc = t.nc = (size_t)cut.n_chunks + 2;
    HIPCHK(ctx, table(B[B_CFLAGS], nc * 4, C.flags)); HIPCHK(ctx, table(B[B_IL], nc * 4, C.il)); HIPCHK(ctx, table(B[B_NCOUNT], nc * 4, C.ncount)); HIPCHK(ctx, table(B[B_NMAP], nc * NMAP_WORDS * 4, C.nmap));
    HIPCHK(ctx, table(B[B_SCAP], nc * MAX_STREAMS * 4, C.scap)); HIPCHK(ctx, table(B[B_SOFF], nc * MAX_STREAMS * 8, C.soff)); HIPCHK(ctx, table(B[B_SSIZE], nc * MAX_STREAMS * 4, C.ssize));
    HIPCHK(ctx, table(B[B_XSIZE], nc * 4, C.xsize)); HIPCHK(ctx, table(B[B_YSIZE], nc * 4, C.ysize)); HIPCHK(ctx, table(B[B_QBASE], nc * 8, C.qbase)); HIPCHK(ctx, table(B[B_SBASE], nc * 8, C.sbase)); HIPCHK(ctx, table(B[B_PTOT], nc * sizeof(U4), C.ptot));
    HIPCHK(ctx, table(B[B_IMGSIZE], nc * 8, C.img_size)); HIPCHK(ctx, table(B[B_IMGOFF], nc * 8, C.img_off)); HIPCHK(ctx, table(B[B_CTOTAL], nc * 8, t.ctot)); HIPCHK(ctx, table(B[B_CBASE], nc * 8, t.cbase));
    HIPCHK(ctx, table(B[B_CTOTALN], nc * 8, t.ctot_n)); HIPCHK(ctx, table(B[B_CBASEN], nc * 8, t.cbase_n)); HIPCHK(ctx, table(B[B_LAYOUT], nc * sizeof(Layout), t.L)); HIPCHK(ctx, table(B[B_OVB], t.nr / 2 + 16, t.ovb));
    HIPCHK(ctx, B[B_HSTATS].ensure(sizeof(HdrStats) + 8192)); HIPCHK(ctx, table(ctx->d_hdr, sizeof(DevHeader), t.D)); HIPCHK(ctx, table(B[B_OVRAW], (size_t)(b.is_pe ? cut.n_units : 0) * 2 + 64, t.ovraw));
    HIPCHK(ctx, B[B_SCANTMP2].ensure(std::max<size_t>(4096, (t.nr / SCAN_TILE + 2) * 16 + (nc / SCAN_TILE + 2) * 8)));
    t.catbytes = (size_t)cut.total_bases + 64 * nc + 256; HIPCHK(ctx, table(B[B_QCAT], t.catbytes, t.qcat));
    HIPCHK(ctx, table(B[B_SPK], (t.catbytes >> 4) * 4 + 64, t.spk)); HIPCHK(ctx, table(B[B_SNM], (t.catbytes >> 4) * 2 + 64, t.snm));     // the tight 2-bit stream and its N mask, which either packer fills
    // per-chunk accumulators of the read-0 / mate comparisons (CF_ALL): all ones; k_chunk_flags_b makes the flag words from them.  The tile gather
    // fills them itself (and the flags follow it); the byte-wise path needs the flags first (overlap search on the text, stored prefix).
    HIPCHK(ctx, table(B[B_ADJ], 3 * nc * 4, t.cbits)); t.cfail = t.cbits + nc; t.redo = t.cfail + nc;
    // the position coder's per-(chunk, stream, 32768-position segment) tables: match counts and last matches are left by the gather
    const uint32_t pc_max_steps = (cut.max_chunk_bases + 4095u) / 4096u; t.n_seg = std::max(1u, (pc_max_steps + PC_SEG_STEPS - 1) / PC_SEG_STEPS);
    const size_t nsb = t.nsb = nc * MAX_STREAMS * (size_t)t.n_seg;
    HIPCHK(ctx, table(B[B_SEGB], nsb * 4, t.segb)); HIPCHK(ctx, table(B[B_SEGC], nsb * 4, t.segc)); HIPCHK(ctx, table(B[B_SEGM], nsb * 4, t.segm));
    return RFQ_OK;
}
// ---- phase 3: header (first batch) - made beside the main stream, on it, or the dense order only - and the parsed names in front of the gather
static int enc_header(rfq_ctx* ctx, EncBatch& b, const EncCut& cut, EncTables& t, EncForm& f) {
    hipStream_t S = ctx->stream;
    // SE: nothing before the gather needs the file header, so the (small, serial) header kernels of a first batch run on the aux
    // stream beside chunk ids / flags / prefix scans; PE needs it for the interleave test right away.
    const bool make_header = f.make_header = !ctx->have_hdr;
    const bool hdr_aside = f.hdr_aside = make_header && !b.is_pe && ctx->aux_ready();
    hipStream_t HS = hdr_aside ? ctx->aux : S;
    if (hdr_aside) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(HS, ctx->ev_fork, 0)); }
    ctx->timer.begin("header", S);
    if (!f.fast) hipLaunchKernelGGL(k_chunk_ids, dim3((cut.max_reads + 255) / 256, cut.n_chunks), dim3(256), 0, S, t.C, t.R);   // (a read's chunk: only the byte-wise path's k_overlap_apply asks)
    // parsed names ahead of the gather: chunk 0's for the file header of a first batch; every read's on the byte-wise path
    const uint32_t c0_reads = std::max(1u, std::min(cut.max_reads, cut.reads_used));
    if (!f.fast) hipLaunchKernelGGL(k_read_table, dim3((cut.n_reads + 255) / 256), dim3(256), 0, S, b.T, t.R, cut.n_reads);
    else if (make_header) hipLaunchKernelGGL(k_read_table, dim3((c0_reads + 255) / 256), dim3(256), 0, S, b.T, t.R, c0_reads);
    if (hdr_aside) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(HS, ctx->ev_fork, 0)); }
    HdrStats* H = ctx->b[B_HSTATS].as<HdrStats>();
    const uint32_t hb = std::min<uint32_t>(1024, (c0_reads + 3) / 4);
    if (make_header) {
        hipLaunchKernelGGL(k_hdr_init, dim3(1), dim3(128), 0, HS, H);
        hipLaunchKernelGGL(k_hdr_stats, dim3(hb), dim3(256), 0, HS, b.T, t.R, (const uint32_t*)t.C.first, H);
        hipLaunchKernelGGL(k_hdr_q0, dim3(1), dim3(64), 0, HS, b.T, H);
        hipLaunchKernelGGL(k_hdr_pass2, dim3(hb), dim3(256), 0, HS, b.T, t.R, (const uint32_t*)t.C.first, H);
        if (b.is_pe) hipLaunchKernelGGL(k_hdr_pe, dim3((c0_reads / 2 + 255) / 256), dim3(256), 0, HS, b.T, t.R, (const uint32_t*)t.C.first, H);
        hipLaunchKernelGGL(k_hdr_finalize, dim3(1), dim3(64), 0, HS, b.T, H, t.D, b.is_pe ? 1 : 0, b.dst);
        if (f.fast) { hipLaunchKernelGGL(k_dense_order, dim3(1), dim3(64), 0, HS, (const HdrStats*)H, t.D); ctx->dense_ok = true; }
        KCHK(ctx, "k_hdr_*");
        if (hdr_aside) HIPCHK(ctx, hipEventRecord(ctx->ev_mid, HS));
    } else if (f.fast && !ctx->dense_ok) {
        // a header that was set, not made (rfq_set_header: a worker of a multi-GPU queue, a later file): which coded values are frequent is taken from this batch's chunk
        // 0
        hipLaunchKernelGGL(k_hdr_init, dim3(1), dim3(128), 0, S, H);
        hipLaunchKernelGGL(k_hdr_stats, dim3(hb), dim3(256), 0, S, b.T, t.R, (const uint32_t*)t.C.first, H);
        hipLaunchKernelGGL(k_dense_order, dim3(1), dim3(64), 0, S, (const HdrStats*)H, t.D);
        ctx->dense_ok = true;
        HIPCHK(ctx, ctx->fetch(ctx->h_hdr.dense, (const uint8_t*)t.D + offsetof(DevHeader, dense), 4, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
    }
    if (make_header && f.fast) {
        // the tile gather is instantiated by the header (match masks for <= 4 coded quality values, bytes otherwise): a first batch waits for it here
        if (hdr_aside) HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_mid, 0));
        HIPCHK(ctx, ctx->fetch(&ctx->h_hdr, t.D, sizeof(DevHeader), S));
        { DevStatus h2; HIPCHK(ctx, ctx->fetch(&h2, b.dst, sizeof h2, S)); HIPCHK(ctx, ctx->fetch_sync(S)); b.hs.err |= h2.err; b.hs.err_read = h2.err_read; b.hs.err_key = h2.err_key; }
    }
    ctx->timer.end(S);
    if (f.fast && make_header) { const int rc = header_errors(ctx, b, f); if (rc) return rc; }
    if (f.fast) enc_form(ctx, cut, f, true);
    return RFQ_OK;
}
// the chunks' image sizes (exact = 0: their upper bounds, from the streams' plans; 1: from the coded streams) and their prefix
static void chunk_layout(hipStream_t Q, const EncBatch& b, const EncCut& cut, const EncTables& t, uint64_t* tmp, int exact) {
    hipLaunchKernelGGL(k_chunk_layout, dim3((cut.n_chunks + 63) / 64), dim3(64), 0, Q, b.T, t.R, t.C, (const DevHeader*)t.D, t.L, cut.n_chunks, exact, b.dst);
    scan_exclusive<uint64_t>(Q, t.C.img_size, t.C.img_off, cut.n_chunks, tmp, 1);
}
// ---- the tile gather, whole: clear list, chunk bases, plane bookkeeping, k_gather2's phases, the quality streams' plan, the second chain on the aux stream
static int enc_gather_tiles(rfq_ctx* ctx, const EncBatch& b, const EncCut& cut, EncTables& t, EncForm& f, AuxGuard& guard) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    const uint32_t np = cut.reads_used / 2;
    if (b.mirrored && f.masks && !G2_SE_OK) return RFQ_AGAIN_MIRROR;         // (a build without k_gather2<true, 1>: the generic match-mask form does not check stream 1)
    // every table of the batch that starts all-zero / all-ones, in one launch (k_clear_list)
    uint8_t *rflag, *rn; HIPCHK(ctx, table(B[B_RFLAG], (t.nr + 15) & ~(size_t)15, rflag)); HIPCHK(ctx, table(B[B_RN], (t.nr + 15) & ~(size_t)15, rn));
    ClearList z; memset(&z, 0, sizeof z);
    if (!(z.add(t.cbits, 2 * t.nc * 4, 0xFFFFFFFFu) && z.add(t.C.ncount, t.nc * 4, 0u) && z.add(t.C.nmap, t.nc * NMAP_WORDS * 4, 0u) && z.add(t.segb, t.nsb * 4, 0u) &&
          z.add(t.segm, t.nsb * 4, 0u) && z.add(t.segc, t.nsb * 4, 0xFFFFFFFFu) && z.add(rflag, t.nr, 0u) && z.add(rn, t.nr, 0u)))
        return rfq_fail(ctx, RFQ_E_HIP, "internal: more than %d regions in one clear list", CLEAR_MAX);
    clear_list(S, z);
    ctx->timer.begin("chunk_flags", S);
    hipLaunchKernelGGL(k_chunk_bases, dim3((cut.n_chunks + 255) / 256), dim3(256), 0, S, t.R, t.C, cut.n_chunks, 1);
    if (f.hdr_aside) HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_mid, 0));    // from here on everything needs the header (major quality, flags, the mates' name2 rule)
    ctx->timer.end(S);

    // (a marker, not a phase: k_gather2 leaves match masks instead of quality bytes - tests and the bench look for it)
    if (f.masks) { ctx->timer.begin("quality_masks", S); ctx->timer.end(S); }
    ctx->timer.begin("gather", S);                                          // (which formulation ran: tests and the bench look at it)
    const size_t nld = (size_t)(cut.total_bases >> 4) + cut.reads_used + 16;
    const size_t lnb_cap = B[B_LNB].cap;
    uint32_t* lpk; uint16_t* lnb; HIPCHK(ctx, table(B[B_LPK], nld * 4, lpk)); HIPCHK(ctx, table(B[B_LNB], nld * 2, lnb));
    // lnb, the loose slots' N bits, is all-zero between batches: the gather stores only the words that hold a bit, k_nbits_cleanup (enc_coders) zeroes those again.  A buffer
    // that has grown or that a call left between here and its cleanup (an error, RFQ_AGAIN_*, a repeat of the batch) is cleared whole; dirty from here until this call's
    // cleanup is queued.
    if (B[B_LNB].cap != lnb_cap) ctx->lnb_dirty = true;
    if (ctx->lnb_dirty) HIPCHK(ctx, hipMemsetAsync(lnb, 0, B[B_LNB].cap, S));
    ctx->lnb_dirty = true;
    const uint32_t K = 1u << f.kshift;
    const uint32_t bx = grid_x_for(cut.n_chunks, (cut.max_reads + K - 1) / K, 6u * ctx->n_cu);      // (26 KB of LDS: six workgroups per CU)
    // dynamic LDS of k_gather2: the staged text of K of the batch's longest records (+ slack), read 0's name / strand line, and - match-mask mode - three
    // bit planes of K of the longest reads.  Six workgroups per CU need <= 26.8 KB each (measured: with five the kernel is 10 % slower).
    const uint32_t text4 = (uint32_t)((((uint64_t)cut.max_rec << f.kshift) + 64u + 15u) / 16u) + 8u;
    G2Planes M; M.planes = nullptr; M.rare = nullptr; M.pstride = 0; M.nd = 0; M.mirror_err = b.mirrored ? &b.dst->err : (uint32_t*)nullptr; M.pw = (uint32_t)((((uint64_t)cut.max_len << f.kshift) + 31u) / 32u) + 2u;
    auto dyn_of = [&](uint32_t nd_) -> uint32_t { return text4 * 16u + (G2_REFN + G2_REFS + 32u) + 4u * nd_ * M.pw; };
    if (f.masks) {
        // dense planes: three if the workgroup still fits six to a CU (26.8 KB of LDS each: with five the kernel is 10 % slower), else two
        M.nd = std::min<uint32_t>(ctx->h_hdr.n_normal, 3u);
        if (M.nd == 3u && dyn_of(3u) + 64u > 26880u) M.nd = 2u;
        // five planes laid out by the buffer's capacity (so that the planes' places are fixed while the buffer is), + rare[n_chunks] behind them
        const size_t need_w = (t.catbytes >> 5) + 16, extra_w = t.nc * (1u + G2_RARE_LIST) / G2_PLANES + 16;
        if (B[B_QPLANE].cap / 4 / G2_PLANES < need_w + extra_w || ctx->qplane_stride < need_w) {
            HIPCHK(ctx, B[B_QPLANE].ensure((need_w + extra_w) * G2_PLANES * 4)); ctx->qplane_stride = B[B_QPLANE].cap / 4 / G2_PLANES - extra_w;
                    ctx->qplane_dirty = true;
        }
        if ((ctx->qplane_stride + extra_w) * G2_PLANES * 4 > B[B_QPLANE].cap) { ctx->qplane_stride = B[B_QPLANE].cap / 4 / G2_PLANES - extra_w;
                ctx->qplane_dirty = true; }
        uint32_t dmask = 0; for (uint32_t d = 0; d < M.nd; d++) dmask |= 1u << (ctx->h_hdr.dense[d] & 7u);
        if (ctx->qplane_mask & ~dmask) ctx->qplane_dirty = true;        // (a plane that was stored whole is now set bit by bit: it has to start all-zero)
        ctx->qplane_mask = dmask;
        M.planes = B[B_QPLANE].as<uint32_t>(); M.pstride = ctx->qplane_stride; M.rare = M.planes + G2_PLANES * M.pstride;
        if (ctx->qplane_dirty) HIPCHK(ctx, hipMemsetAsync(M.planes, 0, ((size_t)M.pstride * G2_PLANES + t.nc * (1u + G2_RARE_LIST)) * 4, S));
        ctx->qplane_dirty = true; ctx->qplane_nd = M.nd;                // (dirty until this call's cleanup is queued)
    }
    t.qplane = f.masks ? M.planes : nullptr;
    const uint32_t dyn = dyn_of(M.nd) + ctx->opt.g2_pad; (void)dyn;   // (the interpreter's launch macro takes its dynamic LDS from a buffer of its own)
    // phase 1: every chunk, names parsed on the way, mates taken for interleaved wherever the header allows; then the flag words; then phase 2 for the
    // (rare) chunks whose interleave test failed somewhere: their workgroups are the only ones of that launch that do not return at once
    for (int phase = 1; phase <= (b.is_pe ? 2 : 1); phase++) {
        const uint32_t* only = phase == 2 ? (const uint32_t*)t.redo : (const uint32_t*)nullptr;
        if (phase == 2) hipLaunchKernelGGL(k_gather_redo_reset, dim3(cut.n_chunks), dim3(64), 0, S, only, t.segm, t.segc, t.n_seg,
                                           f.masks ? M.planes : (uint32_t*)nullptr, M.pstride, (const DevHeader*)t.D, M.nd, (const uint32_t*)t.R.pq, (const uint32_t*)t.C.first, (const uint64_t*)t.C.qbase,
                                           lnb, (const uint8_t*)rn);
        if (f.masks) hipLaunchKernelGGL(k_mask_bounds, dim3(cut.n_chunks), dim3(64), 0, S, (const uint32_t*)t.R.pq, (const uint32_t*)t.C.first, (const uint64_t*)t.C.qbase,
                M.planes, M.pstride, (const DevHeader*)t.D, M.nd, bx, only);
#define RFQ_G2_ARGS b.T, t.R, (const uint32_t*)t.C.first, (const uint64_t*)t.C.qbase, (const DevHeader*)t.D, t.qcat, lpk, lnb, rflag, \
                    rn, t.segm, t.segc, t.n_seg, f.kshift, t.cbits, t.cfail, only, text4, M
        // (single-end input with match masks: the instantiation without mates - 132 spilled SGPRs instead of 182, no VGPR in scratch; the byte-stream form of it
        // spills 64 VGPRs instead and is not used)
        if (f.masks && !b.is_pe && G2_SE_OK) hipLaunchKernelGGL((k_gather2<true, 0>), dim3(bx, cut.n_chunks), dim3(256), dyn, S, RFQ_G2_ARGS);
        // (two files: through one line table - the fact is the instantiation's, with its proof - or with a table each)
        else if (f.masks && b.a->paired == RFQ_PE_TWO_FILES && G2_SE_OK && b.mirrored) hipLaunchKernelGGL((k_gather2<true, 1, true>), dim3(bx, cut.n_chunks), dim3(256), dyn, S, RFQ_G2_ARGS);
        else if (f.masks && b.a->paired == RFQ_PE_TWO_FILES && G2_SE_OK) hipLaunchKernelGGL((k_gather2<true, 1>), dim3(bx, cut.n_chunks), dim3(256), dyn, S, RFQ_G2_ARGS);
        else if (f.masks) hipLaunchKernelGGL(k_gather2<true>, dim3(bx, cut.n_chunks), dim3(256), dyn, S, RFQ_G2_ARGS);
        else hipLaunchKernelGGL(k_gather2<false>, dim3(bx, cut.n_chunks), dim3(256), dyn, S, RFQ_G2_ARGS);
#undef RFQ_G2_ARGS
        if (phase == 1) hipLaunchKernelGGL(k_chunk_flags_b, dim3(cut.n_chunks), dim3(64), 0, S, t.R, t.C, (const DevHeader*)t.D, b.is_pe ? 1 : 0, (const uint32_t*)t.cbits,
                (const uint32_t*)t.cfail, t.redo);
    }
    // the quality streams' scratch plan needs nothing else: the position coder can start as soon as the host has sized its arena
    // The arenas of the coded streams and the image are sized BEFORE their sizes exist (what the context holds from earlier batches, or a guess from the bases): no
    // read-back between the gather and the coders, none behind the second chain.  A total beyond its arena raises DE_SCRATCH(N)_SMALL on the device - the coders and
    // the assembler leave at once - and the batch is repeated with room (RFQ_RETRY_ROOM: once per context as a rule, the arenas keep their size).
    // (the header tells the two shapes apart: a file with at most four coded quality values - match masks - codes a few percent of its positions; one with
    // forty codes most of them, a byte or so each)
    HIPCHK(ctx, table(B[B_SCRATCH], std::max<size_t>(B[B_SCRATCH].cap, (size_t)(f.masks ? cut.total_bases / 8 : cut.total_bases + cut.total_bases / 4) + t.nc * 4096 + 256), t.scratch));
    HIPCHK(ctx, table(B[B_SCRATCHN], std::max<size_t>(B[B_SCRATCHN].cap, (size_t)(cut.total_bases / 64) + t.nc * 1024 + 256), t.scratch_n));
    hipLaunchKernelGGL(k_stream_plan, dim3(cut.n_chunks), dim3(64), 0, S, t.R, t.C, (const DevHeader*)t.D, t.ctot, t.ctot_n, cut.n_chunks, (const uint32_t*)t.segm, t.n_seg, 1);
    scan_exclusive<uint64_t>(S, t.ctot, t.cbase, cut.n_chunks, (uint64_t*)t.scantmp, 1);
    hipLaunchKernelGGL(k_enc_totals, dim3(1), dim3(64), 0, S, t.C, (const uint64_t*)t.cbase, cut.n_chunks, 0, b.dst, (uint64_t)B[B_SCRATCH].cap);
    // Second chain (aux stream), beside the position coder: overlap search on the loose slots the gather has just left, stored prefix, sequence packer
    // (tight 2-bit stream + N mask + N counts), the N streams' plan, the image's upper bound.  These are chains of small latency-bound kernels
    // and a search that is VALU-bound; the coder hides them.
    const bool aux_chain = f.aux_chain = ctx->aux_ready() && !ctx->opt.one_stream; hipStream_t A = aux_chain ? ctx->aux : S;
    if (aux_chain) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(A, ctx->ev_fork, 0)); guard.armed = true; }
    if (b.is_pe) {
        const OvLoose Z = { (const uint32_t*)t.R.pq, (const uint32_t*)lpk, (const uint16_t*)lnb, (const uint8_t*)rflag, (const uint8_t*)rn };
        const uint32_t ob = std::min<uint32_t>((np + 255) / 256, 65535u * 16u);
        // (rows of 160 bases where no read is longer: sixteen resident waves per CU instead of twelve)
        if (cut.max_len <= 160u) hipLaunchKernelGGL((k_overlap<true, 160u>), dim3(ob), dim3(256), 0, A, b.T, Z, t.ovraw, np);
        else hipLaunchKernelGGL(k_overlap<true>, dim3(ob), dim3(256), 0, A, b.T, Z, t.ovraw, np);
        // The search and the position coder are both VALU-bound: side by side they only share the issue slots, and the latency-bound chain behind the search
        // (stored prefix -> sequence packer -> N plan -> N coder) then runs alone, with nothing to hide its round trips (round 4's timeline: coder 1.6 ms and
        // search 2.5 ms together, then 1.9 ms of that chain on an empty device).  The coder waits for the search instead and runs beside the chain
        // (4.4 -> 4.1 ms for the stage.  The packer beside the coder still takes twice its time alone - the coder's single-wave workgroups take the slots
        // that free up - and on a stream of the highest priority it is the other way round, 3.1 ms for the coder: the two kernels take turns, in either order).
    }
    // (the coder waits for the search only: the stored prefix behind it is bound by memory and shares the device well - 3.55 -> 3.48 ms for the phase)
    if (aux_chain) { HIPCHK(ctx, hipEventRecord(ctx->ev_ovl, A)); f.coder_waits = true; }
    hipLaunchKernelGGL(k_chunk_prefix, dim3(cut.n_chunks), dim3(256), 0, A, b.T, t.R, t.C, (const DevHeader*)t.D, (const int16_t*)t.ovraw, t.ovb);
    {
        const uint32_t max_len = cut.max_rec / 2u;                         // (a record holds its sequence twice over: bases and qualities)
        // reads per step of k_seqpack: as many as keep the step's tight dwords inside its owner table (a read of L bases owns at most L / 16 + 1)
        uint32_t rshift = 8; while (rshift && ((uint64_t)(max_len / 16u + 1u) << rshift) > SP_OWN) rshift--;
        uint32_t sx = grid_x_for(cut.n_chunks, (cut.max_reads >> rshift) + 1u, 8u * ctx->n_cu);
        hipLaunchKernelGGL(k_seqpack, dim3(sx, cut.n_chunks), dim3(256), aux_chain ? ctx->opt.sp_pad : 0u, A, (const uint32_t*)t.R.pq, (const uint32_t*)t.R.sd, (const U4*)t.C.ptot,
                (const uint32_t*)t.C.first, (const uint32_t*)t.C.il, (const int8_t*)t.ovb, (const DevHeader*)t.D,
                           (const uint64_t*)t.C.sbase, (const uint32_t*)lpk, (const uint16_t*)lnb, (const uint8_t*)rn, t.spk, t.snm,
                           t.C.ncount, t.C.nmap, t.segm, t.segc, t.n_seg, rshift);
    }
    uint64_t* tmp2 = B[B_SCANTMP2].as<uint64_t>() + (t.nr / SCAN_TILE + 2) * 2;   // (behind the U4 scan's part of the buffer)
    hipLaunchKernelGGL(k_stream_plan, dim3(cut.n_chunks), dim3(64), 0, A, t.R, t.C, (const DevHeader*)t.D, t.ctot, t.ctot_n, cut.n_chunks, (const uint32_t*)t.segm, t.n_seg, 2);
    scan_exclusive<uint64_t>(A, t.ctot_n, t.cbase_n, cut.n_chunks, tmp2, 1);
    chunk_layout(A, b, cut, t, tmp2, 0);
    hipLaunchKernelGGL(k_enc_totals, dim3(1), dim3(64), 0, A, t.C, (const uint64_t*)t.cbase_n, cut.n_chunks, 2, b.dst, (uint64_t)B[B_SCRATCHN].cap);
    KCHK(ctx, "k_gather2");
    ctx->timer.end(S);
    return RFQ_OK;
}
// ---- the byte-wise gather, whole.  It writes the stored bases themselves, so chunk flags, the overlap search (on the text) and the stored prefix come first
static int enc_gather_bytes(rfq_ctx* ctx, EncBatch& b, const EncCut& cut, EncTables& t, EncForm& f) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    uint64_t* const tmp = (uint64_t*)t.scantmp;
    HIPCHK(ctx, hipMemsetAsync(t.cbits, 0xFF, 2 * t.nc * 4, S));
    ctx->timer.begin("chunk_flags", S);
    hipLaunchKernelGGL(k_chunk_bases, dim3((cut.n_chunks + 255) / 256), dim3(256), 0, S, t.R, t.C, cut.n_chunks, 1);
    if (f.hdr_aside) HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_mid, 0));    // from here on everything needs the header (major quality, flags, the mates' name2 rule)
    const uint32_t fbx = std::max(1u, std::min<uint32_t>((cut.max_reads + 255) / 256, std::max(1u, 4096u / cut.n_chunks)));
    hipLaunchKernelGGL(k_chunk_flags_a, dim3(fbx, cut.n_chunks), dim3(256), 0, S, b.T, t.R, t.C, (const DevHeader*)t.D, b.is_pe ? 1 : 0, t.cbits, t.cfail);
    hipLaunchKernelGGL(k_chunk_flags_b, dim3(cut.n_chunks), dim3(64), 0, S, t.R, t.C, (const DevHeader*)t.D, b.is_pe ? 1 : 0, (const uint32_t*)t.cbits, (const uint32_t*)t.cfail,
            (uint32_t*)nullptr);
    if (b.is_pe) {
        const OvLoose noz = { nullptr, nullptr, nullptr, nullptr, nullptr };
        const uint32_t ob = std::min<uint32_t>((cut.n_units + 255) / 256, 65535u * 16u);
        hipLaunchKernelGGL(k_overlap<false>, dim3(ob), dim3(256), 0, S, b.T, noz, t.ovraw, cut.n_units);
    }
    // the stored-base prefix (it needs the mates' overlaps): k_overlap_apply, per-read prefix inputs, their scan, the chunks' bases in the tight streams
    const uint32_t np = cut.reads_used / 2; U4* const pvin = B[B_PVIN].as<U4>();
    if (b.is_pe) hipLaunchKernelGGL(k_overlap_apply, dim3((np + 255) / 256), dim3(256), 0, S, t.R, t.C, (const DevHeader*)t.D, (const int16_t*)t.ovraw, t.ovb, np);
    hipLaunchKernelGGL(k_pv_in, dim3((cut.n_reads + 255) / 256), dim3(256), 0, S, b.T, t.R, pvin, cut.n_reads);
    scan_exclusive<U4>(S, pvin, t.R.pv, cut.n_reads, (U4*)t.scantmp, 1);
    hipLaunchKernelGGL(k_chunk_bases, dim3((cut.n_chunks + 255) / 256), dim3(256), 0, S, t.R, t.C, cut.n_chunks, 2);
    hipLaunchKernelGGL(k_chunk_ptot, dim3((cut.n_chunks + 255) / 256), dim3(256), 0, S, t.R, t.C, cut.n_chunks);
    KCHK(ctx, "k_chunk_flags");
    ctx->timer.end(S);

    ctx->timer.begin("gather_bytes", S);                                    // (which formulation ran: tests and the bench look at it)
    HIPCHK(ctx, hipMemsetAsync(t.C.ncount, 0, t.nc * 4, S)); HIPCHK(ctx, hipMemsetAsync(t.C.nmap, 0, t.nc * NMAP_WORDS * 4, S));
    HIPCHK(ctx, hipMemsetAsync(t.segb, 0, t.nsb * 4, S)); HIPCHK(ctx, hipMemsetAsync(t.segm, 0, t.nsb * 4, S));
            HIPCHK(ctx, hipMemsetAsync(t.segc, 0xFF, t.nsb * 4, S));
    uint8_t* scat; HIPCHK(ctx, table(B[B_SCAT], t.catbytes, scat));
    // workgroups per chunk: each takes a contiguous run of reads in tiles of <= 32
    const uint32_t bx = grid_x_for(cut.n_chunks, (cut.max_reads + GT_READS - 1) / GT_READS, 5u * ctx->n_cu);   // (30 KB of LDS: five workgroups per CU)
    hipLaunchKernelGGL(k_gather, dim3(bx, cut.n_chunks), dim3(256), 0, S, b.T, t.R, t.C, (const int8_t*)t.ovb, (const DevHeader*)t.D, t.qcat, scat, t.segm, t.segc, t.n_seg);
    const uint32_t px = grid_x_for(cut.n_chunks, (cut.max_chunk_bases / 16u + 255u) / 256u + 1u, 8u * ctx->n_cu);
    hipLaunchKernelGGL(k_packbytes, dim3(px, cut.n_chunks), dim3(256), 0, S, (const U4*)t.R.pv, (const uint32_t*)t.C.first, (const uint64_t*)t.C.sbase, (const uint8_t*)scat,
                       t.spk, t.snm);
    hipLaunchKernelGGL(k_stream_plan, dim3(cut.n_chunks), dim3(64), 0, S, t.R, t.C, (const DevHeader*)t.D, t.ctot, t.ctot_n, cut.n_chunks, (const uint32_t*)t.segm, t.n_seg, 3);
    scan_exclusive<uint64_t>(S, t.ctot, t.cbase, cut.n_chunks, tmp, 1);
    scan_exclusive<uint64_t>(S, t.ctot_n, t.cbase_n, cut.n_chunks, tmp, 1);
    chunk_layout(S, b, cut, t, tmp, 0);
    hipLaunchKernelGGL(k_enc_totals, dim3(1), dim3(64), 0, S, t.C, (const uint64_t*)t.cbase, cut.n_chunks, 0, b.dst, ~0ull);
    hipLaunchKernelGGL(k_enc_totals, dim3(1), dim3(64), 0, S, t.C, (const uint64_t*)t.cbase_n, cut.n_chunks, 2, b.dst, ~0ull);
    KCHK(ctx, "k_gather");
    // byte-wise path: arenas by their exact sizes (a read-back here), the header's verdict with them
    HIPCHK(ctx, ctx->fetch(&b.hs, b.dst, sizeof b.hs, S));
    if (f.make_header) HIPCHK(ctx, ctx->fetch(&ctx->h_hdr, t.D, sizeof(DevHeader), S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    ctx->timer.end(S);
    { const int rc = header_errors(ctx, b, f); if (rc) return rc; }
    enc_form(ctx, cut, f, true);
    HIPCHK(ctx, table(B[B_SCRATCH], (size_t)b.hs.total_scratch + 256, t.scratch)); HIPCHK(ctx, table(B[B_SCRATCHN], (size_t)b.hs.total_scratch_n + 256, t.scratch_n));
    return RFQ_OK;
}
// groups g0 .. g0 + gn - 1 of the position coder on stream Q (groups 0 .. nqg - 1: the quality values' streams, then the exception group, then the N group)
static int launch_coder(rfq_ctx* ctx, hipStream_t Q, const EncBatch& b, const EncCut& cut, const EncTables& t, const EncForm& f, uint32_t g0, uint32_t gn) {
    if (f.coder_list && g0 == 0 && gn >= f.nqg) {                            // the value streams; what is left of the request (exception group, N group) below
        const uint64_t mb = (uint64_t)((cut.n_chunks + 7) / 8) * 8ull * t.n_seg;
        if (mb > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "batch too large for the position-coder grid");
        hipLaunchKernelGGL(k_pos_coder_list, dim3((uint32_t)mb), dim3(64), std::min<uint32_t>(ctx->h_hdr.n_normal, NPOS_SLOT) * 128u, Q, t.R, t.C, (const DevHeader*)t.D,
                (const uint8_t*)t.qcat, t.scratch, (const uint64_t*)t.cbase, t.segb, (const int*)t.segc, (const uint32_t*)t.segm, t.n_seg, cut.n_chunks, b.dst);
        g0 = f.nqg; gn -= f.nqg;
        if (gn == 0) return RFQ_OK;
    }
    const uint64_t pc_blocks = (uint64_t)((cut.n_chunks + 7) / 8) * 8ull * gn * t.n_seg;
    if (pc_blocks > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "batch too large for the position-coder grid");
    hipLaunchKernelGGL(k_pos_coder, dim3((uint32_t)pc_blocks), dim3(64), 0, Q, t.R, t.C, (const DevHeader*)t.D, (const uint8_t*)t.qcat, (const uint16_t*)t.snm,
                       t.scratch, (const uint64_t*)t.cbase, t.scratch_n, (const uint64_t*)t.cbase_n,
                       t.segb, (const int*)t.segc, (const uint32_t*)t.segm, t.n_seg, cut.n_chunks, f.nqg, g0, gn, b.dst,
                       (const uint32_t*)t.qplane, (uint64_t)ctx->qplane_stride);
    return RFQ_OK;
}
// ---- phase 4: code streams - the position coder, the coordinates, where the image goes, the rare planes' cleanup, the join of the second stream
static int enc_coders(rfq_ctx* ctx, const EncBatch& b, const EncCut& cut, EncTables& t, const EncForm& f) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    HIPCHK(ctx, table(B[B_XS], 3 * t.nr + 64, t.xs)); HIPCHK(ctx, table(B[B_YS], 3 * t.nr + 64, t.ys));
    ctx->timer.begin("pos_coder", S);
    const bool fork_coords = ctx->aux_ready();
    if (f.fast) {
        // the quality / exception streams now; the N streams when the second chain has planned them (its totals come back while the coder runs)
        if (f.coder_waits) HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_ovl, 0));
        { const int rc = launch_coder(ctx, S, b, cut, t, f, 0, f.nqg + 1); if (rc) return rc; }
        // the coordinate coder (one dependent chain of ~100 steps per (axis, chunk)) needs nothing of either chain: behind the coder on the main stream
        hipLaunchKernelGGL(k_coords, dim3(2, cut.n_chunks), dim3(64), 0, S, t.R, t.C, (const DevHeader*)t.D, t.xs, t.ys, b.dst);
    } else if (fork_coords) { HIPCHK(ctx, hipEventRecord(ctx->ev_fork, S)); HIPCHK(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0)); }
    t.hdr_bytes = b.a->emit_header ? ctx->h_hdr.len : 0;
    if (b.a->d_out) { t.img = b.a->d_out; t.img_cap = b.a->out_cap; } else {
        // (tile path: the image's bound is not on the host - what the context holds, or a third of the text to begin with (7/8 of it for a file with many coded quality
        // values); k_assemble checks every chunk against the room)
        const size_t nb_all = b.nbytes[0] + b.nbytes[1];
        const size_t want = f.fast ? std::max<size_t>(ctx->out_img.cap, (f.masks ? nb_all / 3 : nb_all - nb_all / 8) + (1u << 20)) : (size_t)(b.hs.image_bound + t.hdr_bytes + 64);
        HIPCHK(ctx, ctx->out_img.ensure(want)); t.img = ctx->out_img.as<uint8_t>(); t.img_cap = ctx->out_img.cap;
    }
    if (t.hdr_bytes) {
        if (t.img_cap < t.hdr_bytes) return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffer too small for the header");
        HIPCHK(ctx, hipMemcpyAsync(t.img, ctx->h_hdr.bytes, t.hdr_bytes, hipMemcpyHostToDevice, S));
    }
    // byte-wise path: the coordinate coder runs beside the quality streams on the aux stream; tile path: the N streams behind the second chain (which has
    // planned them)
    hipStream_t A2 = (f.fast ? f.aux_chain : fork_coords) ? ctx->aux : S;
    if (f.fast) { const int rc = launch_coder(ctx, A2, b, cut, t, f, f.nqg + 1, 1); if (rc) return rc; }
    else { hipLaunchKernelGGL(k_coords, dim3(2, cut.n_chunks), dim3(64), 0, A2, t.R, t.C, (const DevHeader*)t.D, t.xs, t.ys, b.dst); const int rc = launch_coder(ctx, S, b, cut, t, f, 0, f.nqg + 2); if (rc) return rc; }
    if (A2 != S) { HIPCHK(ctx, hipEventRecord(ctx->ev_join, A2)); HIPCHK(ctx, hipStreamWaitEvent(S, ctx->ev_join, 0)); }
    KCHK(ctx, "k_pos_coder");
    if (f.masks) {                                                          // the rare planes back to all-zero (stream-ordered behind the coder that read them)
        hipLaunchKernelGGL(k_rare_cleanup, dim3(cut.n_chunks), dim3(256), 0, S, t.qplane + G2_PLANES * ctx->qplane_stride, t.qplane, (uint64_t)ctx->qplane_stride,
                           (const DevHeader*)t.D, ctx->qplane_nd, (const uint32_t*)t.R.pq, (const uint32_t*)t.C.first, (const uint64_t*)t.C.qbase);
        ctx->qplane_dirty = false;
    }
    if (f.fast) {                                                           // the loose N bits back to all-zero, behind k_seqpack (the join above) - also where the coders left early
        hipLaunchKernelGGL(k_nbits_cleanup, dim3((cut.reads_used + 4095u) / 4096u), dim3(256), 0, S, B[B_LNB].as<uint16_t>(), (const uint8_t*)B[B_RN].as<uint8_t>(),
                           (const uint32_t*)t.R.pq, cut.reads_used);
        KCHK(ctx, "k_nbits_cleanup");
        ctx->lnb_dirty = false;
    }
    ctx->timer.end(S);
    return RFQ_OK;
}
// ---- exact layout and assemble
static int enc_assemble(rfq_ctx* ctx, const EncBatch& b, const EncCut& cut, EncTables& t) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    ctx->timer.begin("coords+layout", S);
    uint32_t *segd, *segs; HIPCHK(ctx, table(B[B_SEGD], t.nsb * 4, segd)); HIPCHK(ctx, table(B[B_SEGS], t.nsb * 4, segs));
    hipLaunchKernelGGL(k_pos_sizes, dim3(cut.n_chunks), dim3(64), 0, S, t.C, (const DevHeader*)t.D, (const uint32_t*)t.segb, (const uint32_t*)t.segm, t.n_seg, segd, segs);
    chunk_layout(S, b, cut, t, (uint64_t*)t.scantmp, 1);
    hipLaunchKernelGGL(k_enc_totals, dim3(1), dim3(64), 0, S, t.C, (const uint64_t*)t.cbase, cut.n_chunks, 1, b.dst, ~0ull);
    KCHK(ctx, "k_coords");
    ctx->timer.end(S);
    ctx->timer.begin("assemble", S);
    // the line-break bit of the input's tail chunk looks at how far the readers got on their last, failed attempt (see k_assemble): when this
    // call ends the input - at its end or at an empty line - and not at a worker's chunk boundary
    const uint32_t tail_bases = ((b.a->final && !b.a->flush_all) || b.ended) ? b.a->chunk_bases : 0u;
    const uint32_t bpc = grid_x_for(cut.n_chunks, 64u, 8u * ctx->n_cu);       // (no LDS, 28 VGPRs: eight workgroups per CU)
    hipLaunchKernelGGL(k_assemble, dim3(bpc, cut.n_chunks), dim3(256), 0, S, b.T, t.R, t.C, (const DevHeader*)t.D, (const Layout*)t.L,
                       (const uint8_t*)t.qcat, (const uint32_t*)t.spk, (const uint8_t*)t.scratch, (const uint64_t*)t.cbase,
                       (const uint8_t*)t.scratch_n, (const uint64_t*)t.cbase_n,
                       (const uint8_t*)t.xs, (const uint8_t*)t.ys, (const int8_t*)t.ovb, t.img, t.img_cap, t.hdr_bytes,
                       b.a->file_off1, b.a->file_off2, b.a->nolb_from1, b.a->nolb_from2,
                       (const uint32_t*)t.segb, (const uint32_t*)segd, (const uint32_t*)segs, t.n_seg, b.dst,
                       tail_bases, cut.units_used, cut.nlines[0], cut.nlines[1], b.orig_n(0), b.orig_n(1));
    // (a wave per eight reads, three dependent loads each: as many waves as there are groups of eight, not a serial walk per wave)
    // (most files share their names' fixed parts: the workgroups of such chunks leave at once, so the grid stays small - a workgroup loops over its share)
    const uint32_t bx = std::max(1u, std::min<uint32_t>((cut.max_reads + 31) / 32, std::max(1u, 16384u / cut.n_chunks)));
    hipLaunchKernelGGL(k_assemble_names, dim3(bx, cut.n_chunks), dim3(256), 0, S, b.T, t.R, t.C, (const DevHeader*)t.D, (const Layout*)t.L, t.img, t.img_cap, t.hdr_bytes);
    KCHK(ctx, "k_assemble");
    ctx->timer.end(S);
    return RFQ_OK;
}
// ---- the final read-back and its verdict
static int enc_verdict(rfq_ctx* ctx, EncBatch& b, const EncCut& cut, const EncTables& t, const EncForm& f, AuxGuard& guard, rfq_encode_result* res) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b;
    ctx->chunk_off.resize((size_t)cut.n_chunks + 1);
    HIPCHK(ctx, ctx->fetch(ctx->chunk_off.data(), t.C.img_off, ((size_t)cut.n_chunks + 1) * 8, S));
    uint32_t cons[2] = { 0, 0 };
    for (int s = 0; s < b.nstreams; s++) {
        const uint32_t recs = b.a->paired == RFQ_PE_TWO_FILES ? cut.units_used : cut.reads_used;
        if (b.nm) { cons[s] = 0; if (recs) HIPCHK(ctx, ctx->fetch(&cons[s], b.nm->onx[s] + 4 * (size_t)recs - 1, 4, S)); }
        else HIPCHK(ctx, ctx->fetch(&cons[s], b.T.lo[s] + 4 * (size_t)recs, 4, S));
    }
    HIPCHK(ctx, ctx->fetch(&b.hs, b.dst, sizeof b.hs, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    guard.armed = false; ctx->timer.collect();                              // (the second chain was joined in front of the assembler)
    // one line table for two files: the gather's and k_mirror_tail's verdict in front of everything else this read-back says (it was all made from that table)
    if (b.mirrored) { if (b.hs.err & DE_MIRROR_FAIL) return RFQ_AGAIN_MIRROR; b.mirror_proven = true; }
    if (b.hs.err & DE_COORD_RANGE) {
        // RfqCodec::encodeCoords error_exit, src/rfqcodec.cpp:1315-1317: first offender in (chunk, x-before-y, index) order
        const uint32_t c = (uint32_t)(b.hs.coord_key >> 34), axis = (uint32_t)((b.hs.coord_key >> 33) & 1u), i = (uint32_t)(b.hs.coord_key & 0xFFFFFFFFu);
        uint32_t first = 0, ilv = 0, v = 0;
        HIPCHK(ctx, hipMemcpy(&first, t.C.first + c, 4, hipMemcpyDeviceToHost)); HIPCHK(ctx, hipMemcpy(&ilv, t.C.il + c, 4, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(&v, (axis ? t.R.y : t.R.x) + first + (size_t)i * (ilv ? 2 : 1), 4, hipMemcpyDeviceToHost));
        return rfq_fail(ctx, RFQ_E_DATA, "The X/Y coordinate cannot be larger than 2M, but we get: %u", v);
    }
    // (rare: the tail chunk's line-break bits need the normaliser's verdict on a blank line behind the records)
    if ((b.hs.err & DE_TAIL_BLANK) && !b.nm) return RFQ_NEED_NORM;
    if (f.fast && ((b.hs.err & (DE_SCRATCH_SMALL | DE_SCRATCHN_SMALL)) || ((b.hs.err & (1u << 31)) && !b.a->d_out))) {
        // an arena (or the context's own image buffer) sized in advance was too small: now that the sizes are known, make room and repeat the batch
        HIPCHK(ctx, B[B_SCRATCH].ensure((size_t)b.hs.total_scratch + 256)); HIPCHK(ctx, B[B_SCRATCHN].ensure((size_t)b.hs.total_scratch_n + 256));
        if (!b.a->d_out) HIPCHK(ctx, ctx->out_img.ensure((size_t)(b.hs.image_bound + t.hdr_bytes + 64)));
        ctx->retried_room = true; return RFQ_RETRY_ROOM;
    }
    if (b.hs.err & DE_QUAL_OVERFLOW) return rfq_fail(ctx, RFQ_E_UNPINNED, "quality payload exceeds the reference's 1.5x scratch buffer (reference heap overflow, SURVEY.md App. C Q6)");
    if (b.hs.err & DE_CORRUPT) return rfq_fail(ctx, RFQ_E_HIP, "internal: a stream exceeded its scratch capacity");
    if (b.hs.err & (1u << 31)) return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffer too small: need %llu bytes", (unsigned long long)(b.hs.total_image + t.hdr_bytes));
    for (auto& o : ctx->chunk_off) o += t.hdr_bytes;
    res->d_rfq = t.img; res->rfq_len = (size_t)(b.hs.total_image + t.hdr_bytes); res->n_chunks = cut.n_chunks; res->n_reads = cut.reads_used; res->n_bases = cut.total_bases;
    res->consumed1 = (size_t)consumed_of(b, 0, cons[0]); res->consumed2 = b.nstreams == 2 ? (size_t)consumed_of(b, 1, cons[1]) : 0;
    res->h_chunk_off = ctx->chunk_off.data();
    return RFQ_OK;
}
// One attempt: the stages and the checks between them.  RFQ_OK, an error, or what encode_impl / encode_settled / encode_one do next (RFQ_AGAIN_*, with *again; RFQ_RETRY_ROOM; RFQ_NEED_NORM)
// *mirror: 0 - every stream had its own line index; 1 - stream 0's served both and that is not proven: whatever the attempt says does not count; 2 - proven
static int encode_attempt(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res, const NormMap* nm, EncAgain* again, bool scan_only, const uint32_t* skip, bool mirror_ok,
        int* mirror) {
    EncBatch b = {}; EncCut cut = {}; EncTables t = {}; AuxGuard guard = { ctx, false }; int rc;
    struct MirrorOut { const EncBatch& b; int* out; ~MirrorOut() { *out = b.mirrored ? (b.mirror_proven ? 2 : 1) : 0; } } mirror_out = { b, mirror };
    memset(res, 0, sizeof *res); res->input_ended = again->ended ? 1 : 0;
    b.a = a; b.nm = nm; b.skip = skip; b.scan_only = scan_only; b.ended = again->ended; b.unit_cap = again->unit_cap; b.mirror_ok = mirror_ok;
    b.fin = a->final || again->ended || a->flush_all; b.is_pe = a->paired != RFQ_SE;
    if (a->chunk_bases == 0) return rfq_fail(ctx, RFQ_E_ARG, "chunk_bases must be >= 1");
    const int nstreams = b.nstreams = a->paired == RFQ_PE_TWO_FILES ? 2 : 1;
    b.fq[0] = a->d_fq1; b.fq[1] = nstreams == 2 ? a->d_fq2 : nullptr;
    // skip[s] (< 16): leading bytes of stream s that are not part of it (see k_nl_bitmap); a stream that holds nothing else is empty
    b.nbytes[0] = a->n1 > skip[0] ? a->n1 : 0; b.nbytes[1] = nstreams == 2 ? (a->n2 > skip[1] ? a->n2 : 0) : 0;
    for (int s = 0; s < nstreams; s++) {
        if (b.nbytes[s] >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "a FASTQ stream of one batch must be < 4 GiB (got %zu bytes); split at record boundaries",
                b.nbytes[s]);
        if (b.nbytes[s] && !b.fq[s]) return rfq_fail(ctx, RFQ_E_ARG, "null FASTQ pointer");
        if (((uintptr_t)b.fq[s]) & 15u) return rfq_fail(ctx, RFQ_E_ARG, "FASTQ device pointers must be 16-byte aligned");
    }
    ctx->timer.reset();
    ctx->pend.clear(); ctx->pin_used = 0;                                   // (read-backs an earlier call left behind on an error path)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (a marker, not a phase: this is the repeat of a batch whose arenas were too small - tests look for it)
    if (ctx->retried_room) { ctx->timer.begin("retry_room", ctx->stream); ctx->timer.end(ctx->stream); ctx->retried_room = false; }
    // (the same: a batch of this call was repeated because its second stream did not fit the first one's line table - up for the rest of the call, encode_one takes it down:
    // the room repeat or the lazy index's may still come behind it)
    if (ctx->mirror_fell) { ctx->timer.begin("mirror_fallback", ctx->stream); ctx->timer.end(ctx->stream); }
    HIPCHK(ctx, table(ctx->d_status, sizeof(DevStatus), b.dst));            // ---- status block
    HIPCHK(ctx, fresh_status(ctx, b));
    if ((rc = enc_index(ctx, b, cut)) != RFQ_OK) return rc;
    if ((rc = enc_cut(ctx, b, cut, t, res, again)) != RFQ_OK || cut.n_chunks == 0) return rc;   // (no unit, no chunk: the empty result is made)
    if (scan_only) return enc_chunk_ends(ctx, b, cut, t, res);
    EncForm f = {}; enc_form(ctx, cut, f, false);
    if (b.mirrored) {
        // only the tile gather checks stream 1 against the table (reads too long for a tile, RFQ_GATHER=old: the byte-wise gather does not)
        if (!f.fast) return RFQ_AGAIN_MIRROR;
        hipLaunchKernelGGL(k_mirror_tail, dim3(64), dim3(256), 0, ctx->stream, b.fq[0], b.fq[1], (uint32_t)b.nbytes[0], (const uint32_t*)b.T.lo[0], cut.units_used, b.dst);
        KCHK(ctx, "k_mirror_tail");
    }
    if ((rc = enc_tables(ctx, b, cut, t)) != RFQ_OK) return rc;
    if ((rc = enc_header(ctx, b, cut, t, f)) != RFQ_OK) return rc;
    if ((rc = f.fast ? enc_gather_tiles(ctx, b, cut, t, f, guard) : enc_gather_bytes(ctx, b, cut, t, f)) != RFQ_OK) return rc;
    if ((rc = enc_coders(ctx, b, cut, t, f)) != RFQ_OK) return rc;
    if ((rc = enc_assemble(ctx, b, cut, t)) != RFQ_OK) return rc;
    return enc_verdict(ctx, b, cut, t, f, guard, res);
}
// An attempt, and where it read stream 1 through stream 0's line table without that being proven at its end, a second one with an index per stream.  Such a first attempt
// counts for nothing, whatever it returned: an error may be the table's doing, an empty result was never checked; a header it made from chunk 0 is forgotten.  The
// context remembers a real mismatch (mirror_block, until the header is cleared or set: this input's mates are not aligned); an empty result was merely not looked at.
static int encode_impl(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res, const NormMap* nm, EncAgain* again, bool scan_only, const uint32_t* skip) {
    const bool had_hdr = ctx->have_hdr, had_dense = ctx->dense_ok; int mirror = 0;
    const int rc = encode_attempt(ctx, a, res, nm, again, scan_only, skip, !scan_only, &mirror);
    if (mirror != 1 || rc == RFQ_AGAIN_LAZY) return rc;                        // (the lazy index's repeat has produced nothing yet)
    if (!had_hdr) { ctx->have_hdr = false; ctx->hdr_on_device = false; memset(&ctx->h_hdr, 0, sizeof ctx->h_hdr); }
    if (!had_dense) ctx->dense_ok = false;
    if (rc != RFQ_OK) ctx->mirror_block = true;
    ctx->mirror_fell = true; ctx->err.clear();
    const int rc2 = encode_attempt(ctx, a, res, nm, again, scan_only, skip, false, &mirror);
    // (an error leaves the stage timer as it stands: the repeat's marker is collected here, for whoever asks which way the call went)
    if (rc2 < 0 && hipStreamSynchronize(ctx->stream) == hipSuccess) ctx->timer.collect();
    return rc2;
}
// One text to a settled result.  RFQ_RETRY_ROOM starts again from the call's own arguments, three times at the most; the lazy index's repeat and the empty line's stay inside
// the attempt and do not count (the first takes the lazy form away: a second one is an internal error; the second cuts in front of the line, so it cannot come up twice).
static int encode_settled(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res, const NormMap* nm, bool scan_only, const uint32_t* skip) {
    for (int attempt = 0; attempt < 3; attempt++) {
        EncAgain g; int rc, lazy_repeats = 0;
        while ((rc = encode_impl(ctx, a, res, nm, &g, scan_only, skip)) == RFQ_AGAIN_LAZY || rc == RFQ_AGAIN_ENDED)
            if (rc == RFQ_AGAIN_LAZY && ++lazy_repeats > 1) return rfq_fail(ctx, RFQ_E_HIP, "internal: the index without a read-back ran again in the repeat it asked for");
        if (rc != RFQ_RETRY_ROOM) return rc;
    }
    return rfq_fail(ctx, RFQ_E_HIP, "internal: the stream arenas did not settle");
}

// ---- the front end every call on FASTQ text shares (rfq_encode_batch / rfq_scan_batch: encode_one, encode_or_scan; rfq_text_rows)
// The stream pointers may sit at any byte address: they are rounded down to 16 bytes and the bytes in front are skipped by the indexer (skip[s] < 16)
static void align_streams(const rfq_encode_args* a, rfq_encode_args& al, uint32_t (&skip)[2]) {
    al = *a; skip[0] = skip[1] = 0;
    if (a->n1 && a->d_fq1) { skip[0] = (uint32_t)((uintptr_t)a->d_fq1 & 15u); al.d_fq1 = a->d_fq1 - skip[0]; al.n1 = a->n1 + skip[0];
            al.file_off1 = a->file_off1 - skip[0]; }
    if (a->paired == RFQ_PE_TWO_FILES && a->n2 && a->d_fq2) { skip[1] = (uint32_t)((uintptr_t)a->d_fq2 & 15u); al.d_fq2 = a->d_fq2 - skip[1]; al.n2 = a->n2 + skip[1];
            al.file_off2 = a->file_off2 - skip[1]; }
}
// slow path: '\r' line ends or blank lines (src/fastqreader.cpp:94-196): the call's stream(s) rewritten by normalize_stream, a2 = the call on the normalised text
static int normalize_streams(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_args& a2, NormMap& nm) {
    memset(&nm, 0, sizeof nm); a2 = *a;
    const uint8_t* p; size_t pn; int rc;
    if ((rc = normalize_stream(ctx, a->d_fq1, a->n1, a->file_off1, a->final != 0, 0, nm, &p, &pn)) != RFQ_OK) return rc;
    a2.d_fq1 = p; a2.n1 = pn;
    if (a->paired == RFQ_PE_TWO_FILES) {
        if ((rc = normalize_stream(ctx, a->d_fq2, a->n2, a->file_off2, a->final != 0, 1, nm, &p, &pn)) != RFQ_OK) return rc;
        a2.d_fq2 = p; a2.n2 = pn;
    }
    return RFQ_OK;
}
// what one call indexes of a stream (offsets inside one call are 32-bit): streams below `lim` bytes whole, else slices of `slice` bytes
// (RFQ_SLICE_BYTES: test aid - slices of that many bytes, so that the slicing logic runs on small inputs)
#define RFQ_SLICE ((size_t)3 << 30)
static void slice_limits(const rfq_ctx* ctx, size_t& slice, size_t& lim) {
    const size_t slice_env = ctx->opt.slice_bytes;
    slice = slice_env ? slice_env : RFQ_SLICE; lim = slice_env ? slice_env : 0xFFFFFFF0ull - 16;
}
// One call's worth of text (< 4 GiB per stream)
static int encode_one(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res, bool scan_only) {   // (every attempt starts from a cleared *res)
    rfq_encode_args al; uint32_t skip[2];
    align_streams(a, al, skip);
    ctx->mirror_fell = false;
    int rc = encode_settled(ctx, &al, res, nullptr, scan_only, skip);
    if (rc != RFQ_NEED_NORM) return rc;
    NormMap nm; rfq_encode_args a2; const uint32_t noskip[2] = { 0, 0 };
    if ((rc = normalize_streams(ctx, a, a2, nm)) != RFQ_OK) return rc;
    rc = encode_settled(ctx, &a2, res, &nm, scan_only, noskip);
    return rc == RFQ_NEED_NORM ? rfq_fail(ctx, RFQ_E_HIP, "internal: normalised text still needs normalisation") : rc;
}

// Texts of 4 GiB and more per stream (offsets inside one call are 32-bit): the call is cut into slices of RFQ_SLICE bytes per stream.  A slice
// that is not the last one stops at its last full chunk (final = 0) and the next slice starts right behind the bytes it consumed - in
// place, nothing is copied.  Chunk images are appended in order, so the result is the one-shot image.
static int encode_or_scan(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res, bool scan_only) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (a->paired < 0 || a->paired > 2) return rfq_fail(ctx, RFQ_E_ARG, "paired must be RFQ_SE, RFQ_PE_TWO_FILES or RFQ_PE_INTERLEAVED");
    const bool two = a->paired == RFQ_PE_TWO_FILES;
    const size_t slice_env = ctx->opt.slice_bytes; size_t slice, lim;
    slice_limits(ctx, slice, lim);
    if (a->n1 < lim && (!two || a->n2 < lim)) return encode_one(ctx, a, res, scan_only);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    size_t pos1 = 0, pos2 = 0, written = 0; bool first = true;
    std::vector<uint64_t> offs(1, 0), e1, e2; StageSums sums;
    uint32_t chunks = 0; uint64_t reads = 0, bases = 0; int ended = 0; int32_t ub = 0;
    for (;;) {
        const size_t r1 = a->n1 - pos1, r2 = two ? a->n2 - pos2 : 0;
        size_t t1 = std::min(r1, slice), t2 = std::min(r2, slice);
        // Two files of different length: once one file's slice holds all that is left of it, no pair lies beyond it - the other file's slice grows
        // to what is left of ITS file (as far as one call can address), and the call ends the input there like the reference does (it truncates
        // to the shorter file).  (With the other slice left at its size the slice ran as a non-final one, the short file's last records - less
        // than a chunk - were never flushed, and the call failed with "no whole chunk".)
        if (two && (t1 == r1) != (t2 == r2)) { const size_t grow = slice_env ? 64 * slice_env : lim; if (t1 == r1) t2 = std::min(r2, grow); else t1 = std::min(r1, grow);
                }
        const bool last = t1 == r1 && t2 == r2;
        rfq_encode_args s = *a;
        s.d_fq1 = a->d_fq1 + pos1; s.n1 = t1; s.file_off1 = a->file_off1 + pos1;
        if (two) { s.d_fq2 = a->d_fq2 + pos2; s.n2 = t2; s.file_off2 = a->file_off2 + pos2; }
        s.final = last ? a->final : 0; s.flush_all = last ? a->flush_all : 0; s.emit_header = first ? a->emit_header : 0; s.carry_bases = first ? a->carry_bases : 0u;
        if (a->d_out) { s.d_out = a->d_out + written; s.out_cap = a->out_cap > written ? a->out_cap - written : 0; }
        rfq_encode_result r;
        const int rc = encode_one(ctx, &s, &r, scan_only);
        if (rc != RFQ_OK) return rc;
        sums.add(ctx->timer);
        if (scan_only) {
            for (uint32_t c = 0; c < r.n_chunks; c++) { e1.push_back(ctx->scan_end[0][c] + pos1); if (two) e2.push_back(ctx->scan_end[1][c] + pos2); }
        } else if (r.rfq_len) {
            if (!a->d_out) {            // the slice's image sits in the context's result buffer: append it to the call's
                HIPCHK(ctx, ctx->out_acc.ensure_keep(written + r.rfq_len + 64, written, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(ctx->out_acc.as<uint8_t>() + written, r.d_rfq, r.rfq_len, hipMemcpyDeviceToDevice, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            }
            for (uint32_t c = 1; c <= r.n_chunks; c++) offs.push_back(written + r.h_chunk_off[c]);
            if (first && r.n_chunks) offs[0] = r.h_chunk_off[0];
            written += r.rfq_len;
        }
        if (first) ub = r.reserved; else if (r.reserved != ub) ub = 0;      // (scan: the units' common length, if the slices agree on one)
        chunks += r.n_chunks; reads += r.n_reads; bases += r.n_bases; pos1 += r.consumed1; pos2 += r.consumed2; first = false;
        if (r.input_ended) { ended = 1; break; }
        if (last) break;
        if (r.consumed1 == 0) return rfq_fail(ctx, RFQ_E_ARG, "no whole chunk inside %zu bytes of text: chunk_bases is too large for a sliced call", slice);
    }
    sums.publish(ctx->timer);
    res->n_chunks = chunks; res->n_reads = reads; res->n_bases = bases; res->consumed1 = pos1; res->consumed2 = pos2; res->input_ended = ended;
            res->reserved = scan_only ? ub : 0;
    if (scan_only) { ctx->scan_end[0] = e1; ctx->scan_end[1] = e2; return RFQ_OK; }
    ctx->chunk_off = offs; res->h_chunk_off = ctx->chunk_off.data();
    res->rfq_len = written; res->d_rfq = written ? (a->d_out ? a->d_out : ctx->out_acc.as<uint8_t>()) : nullptr;
    return RFQ_OK;
}
extern "C" int rfq_encode_batch(rfq_ctx* ctx, const rfq_encode_args* a, rfq_encode_result* res) { return encode_or_scan(ctx, a, res, false); }
extern "C" int rfq_scan_batch(rfq_ctx* ctx, const rfq_encode_args* a, rfq_scan_result* out) {
    if (!out) return RFQ_E_ARG;
    memset(out, 0, sizeof *out);
    rfq_encode_result r;
    const int rc = encode_or_scan(ctx, a, &r, true);
    if (rc != RFQ_OK) return rc;
    out->n_chunks = r.n_chunks; out->n_reads = r.n_reads; out->consumed1 = r.consumed1; out->consumed2 = r.consumed2; out->input_ended = r.input_ended;
            out->unit_bases = (uint32_t)r.reserved;
    out->h_end1 = r.n_chunks ? ctx->scan_end[0].data() : nullptr;
    out->h_end2 = (r.n_chunks && a->paired == RFQ_PE_TWO_FILES) ? ctx->scan_end[1].data() : nullptr;
    return RFQ_OK;
}
// ---------------------------------------------------------------- steps the rows entry points below share
// a call begins: no stage timed, nothing waiting in the read-back block, the context's device current
static int rows_begin(rfq_ctx* ctx) {
    ctx->timer.reset(); ctx->pend.clear(); ctx->pin_used = 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return RFQ_OK;
}
// the context's verdict block as a fresh Stat: all zero, bad_row (and the text's first_empty, the grouping's bad_unit) all ones - "no such row" under the kernels' atomicMin
template <class Stat> static int rows_stat_fresh(rfq_ctx* ctx, hipStream_t S, Stat** dst) {
    HIPCHK(ctx, ctx->rows_stat.ensure(sizeof(Stat)));
    Stat* const d = *dst = ctx->rows_stat.as<Stat>();
    HIPCHK(ctx, hipMemsetAsync(d, 0, sizeof(Stat), S));
    if constexpr (std::is_same<Stat, TextRowsStat>::value) HIPCHK(ctx, hipMemsetAsync(&d->first_empty, 0xFF, sizeof d->first_empty, S));
    if constexpr (std::is_same<Stat, GroupStat>::value) HIPCHK(ctx, hipMemsetAsync(&d->bad_unit, 0xFF, sizeof d->bad_unit, S));
    HIPCHK(ctx, hipMemsetAsync(&d->bad_row, 0xFF, sizeof d->bad_row, S));
    return RFQ_OK;
}
// output rows of a workgroup of k_text_rows / k_sel_rows: about four 16-byte groups per thread
static uint32_t rows_per(uint32_t row_len) { const uint32_t G = (row_len + 15u) / 16u; return std::max(1u, 1024u / G); }
// workgroups of a names writer (name_blob_write): tiles of TN_TILE bytes, counted from the 16-byte boundary at or below the blob
static int name_blob_blocks(rfq_ctx* ctx, const uint8_t* dst, uint64_t names_len, uint32_t* blocks) {
    const uint64_t span = names_len + ((uintptr_t)dst & 15u), nb = (span + TN_TILE - 1) / TN_TILE;
    if (nb > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "a name blob of %llu bytes is too large for one call", (unsigned long long)names_len);
    *blocks = (uint32_t)nb;
    return RFQ_OK;
}
// room for everything asked for, or nothing is written (A: rfq_text_rows_args, rfq_select_rows_args - the same output fields)
template <class A> static int rows_room(rfq_ctx* ctx, const A* a, uint64_t n_rows, uint64_t names_len, uint32_t max_len) {
    const unsigned long long rowb = (unsigned long long)n_rows * a->row_len;
    if ((n_rows && a->row_len < max_len) || (a->d_bases && a->bases_cap < rowb) || (a->d_quals && a->quals_cap < rowb) || (a->d_lens && a->lens_cap < n_rows) ||
        (a->d_names && a->names_cap < names_len) || (a->d_name_off && a->off_cap < n_rows + 1))
        return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffers too small: need row_len >= %u, %llu bytes per row buffer (at that row_len: %llu), %llu lens, %llu name bytes, %llu offsets",
                        max_len, rowb, (unsigned long long)n_rows * std::max(a->row_len, max_len), (unsigned long long)n_rows, (unsigned long long)names_len,
                        (unsigned long long)n_rows + 1);
    return RFQ_OK;
}
// a call that leaves no rows: the offsets of no names are one zero
static int rows_none(rfq_ctx* ctx, uint64_t* d_name_off) {
    if (d_name_off) HIPCHK(ctx, hipMemsetAsync(d_name_off, 0, 8, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); ctx->timer.collect();
    return RFQ_OK;
}
// no output may lie on an input: the bytes a call can write against the bytes it reads (tail: what the message ends in)
struct Span { const void* p; unsigned long long n; const char* what; };
static bool sel_overlap(const void* a, unsigned long long an, const void* b, unsigned long long bn) {
    if (!a || !b || !an || !bn) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    const uintptr_t a1 = an > UINTPTR_MAX - a0 ? UINTPTR_MAX : a0 + (uintptr_t)an, b1 = bn > UINTPTR_MAX - b0 ? UINTPTR_MAX : b0 + (uintptr_t)bn;
    return a0 < b1 && b0 < a1;
}
template <size_t NO, size_t NI> static int rows_apart(rfq_ctx* ctx, const Span (&outs)[NO], const Span (&ins)[NI], const char* tail) {
    for (const Span& o : outs) for (const Span& i : ins)
        if (sel_overlap(o.p, o.n, i.p, i.n)) return rfq_fail(ctx, RFQ_E_ARG, "the output %s overlaps the input %s%s", o.what, i.what, tail);
    return RFQ_OK;
}
// nor may two outputs of a call that writes several tables lie on each other
template <size_t NO> static int rows_outs_apart(rfq_ctx* ctx, const Span (&outs)[NO]) {
    for (size_t i = 0; i < NO; i++) for (size_t k = i + 1; k < NO; k++)
        if (sel_overlap(outs[i].p, outs[i].n, outs[k].p, outs[k].n)) return rfq_fail(ctx, RFQ_E_ARG, "the output %s overlaps the output %s", outs[i].what, outs[k].what);
    return RFQ_OK;
}
// A workgroup pays for its set-up - a table in LDS it fills or flushes - once, so the grid is capped at `wg_cap` workgroups (at least one) and the steps each takes
// follow from that: `units` units, `per_step` a step and workgroup, the steps clamped to lo .. hi.  The grid is rows_steps_grid of them: beyond hi it grows instead.
static uint64_t rows_steps_for(uint64_t units, uint64_t per_step, uint64_t wg_cap, uint64_t lo, uint64_t hi) {
    const uint64_t per_round = per_step * std::max<uint64_t>(wg_cap, 1u);
    return std::min(std::max((units + per_round - 1u) / per_round, lo), hi);
}
static uint32_t rows_steps_grid(uint64_t units, uint64_t per_step, uint64_t steps) { return (uint32_t)((units + per_step * steps - 1u) / (per_step * steps)); }
// ---- the plan of a compacting call (rfq_select_rows over rows, rfq_merge_rows over pairs): judge, two scans, ONE read-back; the caller refuses or goes on; tables,
// row writer, names writer.  A caller supplies its unit count, its stage names and three launches - the judge, the tables kernel, the row writer - and keeps its own
// argument checks (in its own order: the first refusal met is the one reported), its verdict on the Stat and its result fields.
struct RowsStages { const char* judge; const char* tables; const char* rows; const char* names; };
// A below: rfq_select_rows_args, rfq_merge_rows_args - they end in the same output block (row_len, pad_*, d_bases / bases_cap .. d_name_off / off_cap), as rows_room takes it
template <class A> static bool rows_size_query(const A* o) { return !o->d_bases && !o->d_quals && !o->d_lens && !o->d_names && !o->d_name_off; }
template <class A> static int rows_dst_len(rfq_ctx* ctx, const A* o) { return !rows_size_query(o) && o->row_len == 0 ? rfq_fail(ctx, RFQ_E_ARG, "row_len must be >= 1") : (int)RFQ_OK; }
template <class A> static int rows_dst_named(rfq_ctx* ctx, const A* o, bool named) {
    if (named || (!o->d_names && !o->d_name_off)) return RFQ_OK;
    return rfq_fail(ctx, RFQ_E_ARG, "rows without names (d_name_off == NULL) have no name outputs: d_names / d_name_off must be NULL");
}
// (others4 / what4: the caller's further 4-byte inputs, ORed, and what the message calls them all)
template <class A> static int rows_dst_aligned(rfq_ctx* ctx, const rfq_rows_in* in, const A* o, uintptr_t others4, const char* what4) {
    if (((uintptr_t)in->d_lens | (uintptr_t)o->d_lens | others4) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "%s must be 4-byte aligned", what4);
    if (((uintptr_t)in->d_name_off | (uintptr_t)o->d_name_off) & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_name_off must be 8-byte aligned");
    return RFQ_OK;
}
// the bytes a call can write: its cap, and never more than `units` rows of row_len or the names there are
template <class A> static void rows_dst_spans(const A* o, uint64_t units, uint64_t names_len, Span (&outs)[5]) {
    const unsigned long long rows_out = (unsigned long long)units * o->row_len;
    outs[0] = { o->d_bases, std::min<unsigned long long>(o->bases_cap, rows_out), "d_bases" }; outs[1] = { o->d_quals, std::min<unsigned long long>(o->quals_cap, rows_out), "d_quals" };
    outs[2] = { o->d_lens, std::min<unsigned long long>(o->lens_cap, units) * 4ull, "d_lens" }; outs[3] = { o->d_names, std::min<unsigned long long>(o->names_cap, names_len), "d_names" };
    outs[4] = { o->d_name_off, std::min<unsigned long long>(o->off_cap, units + 1) * 8ull, "d_name_off" };
}
// what the callables handed to rows_judge / rows_write end in, behind their hipLaunchKernelGGL: the launch's error, if it left one
static int launched(rfq_ctx* ctx, const char* what) { KCHK(ctx, what); return RFQ_OK; }
// judge(pos, noff, dst) launches the judging kernel: a kept flag per unit in pos[], the kept name size in noff[] (null: rows without names), the verdict in *dst.
// Both are scanned in place, their totals behind them; *hs, n_out and names_len come back in ONE read-back.  No units: nothing runs, *hs stays zero.
struct RowsJudged { uint32_t* pos = nullptr; uint64_t* noff = nullptr; uint32_t n_out = 0; uint64_t names_len = 0; };
template <class Stat, class Judge> static int rows_judge(rfq_ctx* ctx, uint64_t units, bool named, const char* stage, Judge judge, Stat* hs, RowsJudged* j) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; int rc;
    memset(hs, 0, sizeof *hs);
    if (!units) return RFQ_OK;
    ctx->timer.begin(stage, S);
    Stat* dst = nullptr;
    HIPCHK(ctx, table(B[B_LEN], ((size_t)units + 2) * 4, j->pos));
    if (named) HIPCHK(ctx, table(B[B_P], ((size_t)units + 2) * 8, j->noff));
    HIPCHK(ctx, B[B_SCANTMP].ensure(std::max<size_t>(1024, ((size_t)units / SCAN_TILE + 2) * 16)));
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if ((rc = judge(j->pos, j->noff, dst)) != RFQ_OK) return rc;
    scan_exclusive<uint32_t>(S, j->pos, j->pos, units, B[B_SCANTMP].as<uint32_t>(), 1);
    if (named) scan_exclusive<uint64_t>(S, j->noff, j->noff, units, B[B_SCANTMP].as<uint64_t>(), 1);
    KCHK(ctx, "scan_exclusive");
    ctx->timer.end(S);
    HIPCHK(ctx, ctx->fetch(hs, dst, sizeof *hs, S));
    HIPCHK(ctx, ctx->fetch(&j->n_out, j->pos + units, 4, S));
    if (named) HIPCHK(ctx, ctx->fetch(&j->names_len, j->noff + units, 8, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    return RFQ_OK;
}
// tables(pos, noff, tab, ooff) launches the tables kernel (a rows_tables), rows(o, tab) completes o - vec_in and what else is its own - and launches the row writer;
// names(tab, ooff) writes the name blob along the same table and times its own stages - k_sel_names (rows_names_whole) unless the caller has another (rfq_select_rows
// with a tag).  Ends the call: synchronised, the stage times collected.
template <class A> static int rows_names_whole(rfq_ctx* ctx, const rfq_rows_in* in, const A* a, const RowsJudged& j, const char* stage, const SelRow* tab, const uint64_t* ooff) {
    hipStream_t S = ctx->stream; int rc;
    ctx->timer.begin(stage, S);
    if (a->d_names && j.names_len) {
        uint32_t blocks = 0;
        if ((rc = name_blob_blocks(ctx, a->d_names, j.names_len, &blocks)) != RFQ_OK) return rc;
        hipLaunchKernelGGL(k_sel_names, dim3(blocks), dim3(TN_TPB), 0, S, in->d_names, in->d_name_off, tab, ooff, j.n_out, a->d_names, j.names_len);
        KCHK(ctx, "k_sel_names");
    }
    ctx->timer.end(S);
    return RFQ_OK;
}
template <class A, class Tables, class Rows, class Names> static int rows_write(rfq_ctx* ctx, const rfq_rows_in* in, const A* a, const RowsJudged& j, const RowsStages& st, Tables tables, Rows rows,
        Names names) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; int rc;
    const uint32_t n_out = j.n_out;
    ctx->timer.begin(st.tables, S);
    SelRow* tab = nullptr; uint64_t* ooff = nullptr;
    HIPCHK(ctx, table(B[B_X], (size_t)n_out * sizeof(SelRow), tab));
    if (j.noff) HIPCHK(ctx, table(B[B_Y], ((size_t)n_out + 1) * 8, ooff));
    if ((rc = tables((const uint32_t*)j.pos, (const uint64_t*)j.noff, tab, ooff)) != RFQ_OK) return rc;
    ctx->timer.end(S);
    ctx->timer.begin(st.rows, S);
    if (a->d_bases || a->d_quals) {
        RowsOut o; memset(&o, 0, sizeof o);
        o.sb = in->d_bases; o.sq = in->d_quals; o.bases = a->d_bases; o.quals = a->d_quals;
        o.row_len_in = in->row_len; o.total_in = in->n_rows * in->row_len; o.row_len = a->row_len; o.n_out = n_out;
        o.pad_b4 = a->pad_base * 0x01010101u; o.pad_q4 = a->pad_qual * 0x01010101u;
        o.vec = rows_vec(a->row_len, a->d_bases, a->d_quals); o.per = rows_per(a->row_len);
        if ((rc = rows(o, (const SelRow*)tab)) != RFQ_OK) return rc;
    }
    ctx->timer.end(S);
    if ((rc = names((const SelRow*)tab, (const uint64_t*)ooff)) != RFQ_OK) return rc;
    HIPCHK(ctx, hipStreamSynchronize(S));
    ctx->timer.collect();
    return RFQ_OK;
}
template <class A, class Tables, class Rows> static int rows_write(rfq_ctx* ctx, const rfq_rows_in* in, const A* a, const RowsJudged& j, const RowsStages& st, Tables tables, Rows rows) {
    return rows_write(ctx, in, a, j, st, tables, rows, [&](const SelRow* tab, const uint64_t* ooff) -> int { return rows_names_whole(ctx, in, a, j, st.names, tab, ooff); });
}
// ---- the argument rules the rows calls word alike.  Each is called where its call tests it: the first refusal met is the one reported.
static int rows_pairs_arg(rfq_ctx* ctx, int32_t pairs, uint64_t n) {
    if (pairs != 0 && pairs != 1) return rfq_fail(ctx, RFQ_E_ARG, "pairs must be 0 or 1");
    if (pairs && (n & 1u)) return rfq_fail(ctx, RFQ_E_ARG, "pairs takes rows in pairs (got %llu rows)", (unsigned long long)n);
    return RFQ_OK;
}
static int rows_base_mode_arg(rfq_ctx* ctx, const rfq_rows_in* in) {
    return in->base_mode != RFQ_ROWS_ASCII && in->base_mode != RFQ_ROWS_CODE ? rfq_fail(ctx, RFQ_E_ARG, "bad base_mode %d", in->base_mode) : (int)RFQ_OK;
}
// (asked: rfq_select_rows asks of no rows too, the others of n_rows != 0)
static int rows_src_len_arg(rfq_ctx* ctx, const rfq_rows_in* in, bool asked) { return asked && in->row_len == 0 ? rfq_fail(ctx, RFQ_E_ARG, "the rows' row_len must be >= 1") : (int)RFQ_OK; }
static int rows_len_refusal(rfq_ctx* ctx, uint32_t row_len, unsigned long long row) {
    return rfq_fail(ctx, RFQ_E_ARG, "a read length is negative or greater than row_len = %u (first such row: %llu)", row_len, row);
}
// the bytes a call reads of its rows, in ins[0 .. 5) (rows_dst_spans' mirror); a call appends its own inputs and takes out (p = null) an array it does not read
template <size_t N> static void rows_src_spans(const rfq_rows_in* in, bool named, Span (&ins)[N]) {
    static_assert(N >= 5, "five spans of the rows, then the call's own");
    const unsigned long long n = in->n_rows, rows_in = n * in->row_len;
    ins[0] = { in->d_bases, rows_in, "rows->d_bases" }; ins[1] = { in->d_quals, rows_in, "rows->d_quals" }; ins[2] = { in->d_lens, n * 4ull, "rows->d_lens" };
    ins[3] = { in->d_names, named ? (unsigned long long)in->names_len : 0ull, "rows->d_names" }; ins[4] = { in->d_name_off, named ? (n + 1) * 8ull : 0ull, "rows->d_name_off" };
}
// ---- the path of a deciding call (rfq_judge_rows, rfq_adapter_rows, rfq_dedup_rows: a verdict per unit, no row moved - enc/rows_lanes.h).  A call keeps its own
// argument rules, its *In block and its result fields.  Its histogram starts at zero, rows or not; with no rows that is all the call does (the caller returns)
static int rows_hist_fresh(rfq_ctx* ctx, hipStream_t S, uint64_t* d_hist, uint32_t hist_len, uint64_t n) {
    if (d_hist) HIPCHK(ctx, hipMemsetAsync(d_hist, 0, (size_t)hist_len * 8, S));
    if (!n) HIPCHK(ctx, hipStreamSynchronize(S));
    return RFQ_OK;
}
// Which kernel is the row length's to say: up to 256 bytes a DPP row of 16 lanes holds a unit's row (k16), up to 1024 a wave (k64) - 256 threads, 16 / 4 units at
// a time, `iter` times -, beyond that (or where the call's `general` option is set) a wave per unit walks it (k_long).  The caller's KCHK names the kernel.
template <class In, class Stat> static void rows_launch_by_len(hipStream_t S, bool general, uint32_t row_len, uint64_t units, uint32_t iter,
        void (*k16)(In, Stat*), void (*k64)(In, Stat*), void (*k_long)(In, Stat*), const In& in, Stat* dst) {
    if (general || row_len > 1024u) { hipLaunchKernelGGL(k_long, dim3((uint32_t)units), dim3(64), 0, S, in, dst); return; }
    const auto k = row_len <= 256u ? k16 : k64; const uint32_t per = (row_len <= 256u ? 16u : 4u) * iter;
    hipLaunchKernelGGL(k, dim3((uint32_t)((units + per - 1u) / per)), dim3(256), 0, S, in, dst);
}
// the verdict block back on the host, the stage times collected; a bad length refuses the call
template <class Stat> static int rows_sums_back(rfq_ctx* ctx, hipStream_t S, const Stat* dst, Stat* hs, uint32_t row_len) {
    memset(hs, 0, sizeof *hs);
    HIPCHK(ctx, ctx->fetch(hs, dst, sizeof *hs, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    ctx->timer.collect();
    return hs->err & ROWS_ERR_LEN ? rows_len_refusal(ctx, row_len, hs->bad_row) : (int)RFQ_OK;
}
// ---------------------------------------------------------------- rows -> FASTQ text (-> image): rfq_rows_to_text, rfq_encode_rows of include/rfq_hip.h
// The judged part (k_rows_sizes + one scan per text) ends in ONE read-back - the texts' sizes, the bases, the error bits - and the writer (k_rows_text)
// runs only on rows that passed; what the writer itself finds in the bytes comes back with a second look at the same block.
static int rows_text_impl(rfq_ctx* ctx, const rfq_rows_in* in, int32_t paired, uint8_t* d_out1, size_t cap1, uint8_t* d_out2, size_t cap2, bool size_only,
        rfq_rows_text_result* res) {
    memset(res, 0, sizeof *res);
    if (paired < 0 || paired > 2) return rfq_fail(ctx, RFQ_E_ARG, "paired must be RFQ_SE, RFQ_PE_TWO_FILES or RFQ_PE_INTERLEAVED");
    const bool two = paired == RFQ_PE_TWO_FILES; const int nt = two ? 2 : 1;
    const uint64_t n = in->n_rows;
    if (in->row_len == 0) return rfq_fail(ctx, RFQ_E_ARG, "row_len must be >= 1");
    if (in->base_mode != RFQ_ROWS_ASCII && in->base_mode != RFQ_ROWS_CODE) return rfq_fail(ctx, RFQ_E_ARG, "base_mode must be RFQ_ROWS_ASCII or RFQ_ROWS_CODE");
    if (two && (n & 1u)) return rfq_fail(ctx, RFQ_E_ARG, "RFQ_PE_TWO_FILES takes rows in pairs (got %llu rows)", (unsigned long long)n);
    if (n >= (1ull << 39)) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if (n && (!in->d_bases || !in->d_quals || !in->d_lens || !in->d_name_off || (in->names_len && !in->d_names))) return rfq_fail(ctx, RFQ_E_ARG, "null row / name pointer");
    if (((uintptr_t)in->d_lens & 3u) || ((uintptr_t)in->d_name_off & 7u)) return rfq_fail(ctx, RFQ_E_ARG, "d_lens must be 4-byte and d_name_off 8-byte aligned");
    if ((((uintptr_t)d_out1) | ((uintptr_t)d_out2)) & 15u) return rfq_fail(ctx, RFQ_E_ARG, "output buffers must be 16-byte aligned");
    if (!size_only && two && (d_out1 == nullptr) != (d_out2 == nullptr)) return rfq_fail(ctx, RFQ_E_ARG, "RFQ_PE_TWO_FILES: give both output buffers or none");
    hipStream_t S = ctx->stream; int rc;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    if (n == 0) { ctx->timer.collect(); return RFQ_OK; }
    const uint64_t nrec[2] = { two ? n / 2 : n, two ? n / 2 : 0 };
    RowsIn ri; memset(&ri, 0, sizeof ri);
    ri.bases = in->d_bases; ri.quals = in->d_quals; ri.lens = in->d_lens; ri.names = in->d_names; ri.name_off = in->d_name_off;
    ri.n_rows = n; ri.names_len = in->names_len; ri.row_len = in->row_len; ri.codes = in->base_mode == RFQ_ROWS_CODE ? 1u : 0u;
    ri.qoff = in->qual_offset; ri.qoff4 = in->qual_offset * 0x01010101u;
    ri.vec = rows_vec(in->row_len, in->d_bases, in->d_quals);

    ctx->timer.begin("rows_sizes", S);
    RowsStat* dst = nullptr;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    for (int t = 0; t < nt; t++) HIPCHK(ctx, ctx->rows_off[t].ensure((size_t)(nrec[t] + 2) * 8));
    HIPCHK(ctx, ctx->b[B_SCANTMP].ensure(std::max<size_t>(1024, (size_t)(nrec[0] / SCAN_TILE + 2) * 16)));
    uint64_t* off[2] = { ctx->rows_off[0].as<uint64_t>(), two ? ctx->rows_off[1].as<uint64_t>() : nullptr };
    hipLaunchKernelGGL(k_rows_sizes, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, S, ri, two ? 1u : 0u, off[0], off[1], dst);
    KCHK(ctx, "k_rows_sizes");
    for (int t = 0; t < nt; t++) scan_exclusive<uint64_t>(S, off[t], off[t], nrec[t], ctx->b[B_SCANTMP].as<uint64_t>(), 1);
    KCHK(ctx, "scan_exclusive");
    ctx->timer.end(S);
    RowsStat hs; uint64_t total[2] = { 0, 0 };
    HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
    for (int t = 0; t < nt; t++) HIPCHK(ctx, ctx->fetch(&total[t], off[t] + nrec[t], 8, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    const unsigned long long br = hs.bad_row;
    if (hs.err & RT_ERR_LEN) return rows_len_refusal(ctx, in->row_len, br);
    if (hs.err & RT_ERR_NOFF) return rfq_fail(ctx, RFQ_E_ARG, "the name offsets decrease or end past names_len = %zu (first such row: %llu)", in->names_len, br);
    if (hs.err & RT_ERR_LEN0) return rfq_fail(ctx, RFQ_E_DATA, "a read of no bases (first such row: %llu): an empty sequence line ends the reference's reader", br);
    if (hs.err & RT_ERR_NAME0) return rfq_fail(ctx, RFQ_E_DATA, "a name of no bytes (first such row: %llu)", br);
    res->n1 = (size_t)total[0]; res->n2 = (size_t)total[1]; res->n_reads = n; res->n_bases = hs.n_bases;
    if (size_only) { ctx->timer.collect(); return RFQ_OK; }

    uint8_t* out[2] = { d_out1, two ? d_out2 : nullptr };
    if (d_out1) {
        if (cap1 < total[0] || (two && cap2 < total[1])) {
            const unsigned long long n1 = total[0], n2 = total[1];
            memset(res, 0, sizeof *res);
            return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffers too small: need %llu bytes of text 1 and %llu of text 2", n1, n2);
        }
    } else {
        // (the encoder reads its text in 16-byte groups: a 256-byte aligned start and slack behind the last byte, like its normalised-text buffers)
        for (int t = 0; t < nt; t++) { HIPCHK(ctx, ctx->rows_txt[t].ensure((size_t)total[t] + 64 + 16)); out[t] = ctx->rows_txt[t].as<uint8_t>(); }
    }
    ctx->timer.begin("rows_text", S);
    for (int t = 0; t < nt; t++) {
        if (!total[t]) continue;
        const uint64_t blocks = (total[t] + RT_TILE - 1) / RT_TILE;
        if (blocks > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "a text of %llu bytes is too large for one call", (unsigned long long)total[t]);
        hipLaunchKernelGGL(k_rows_text, dim3((uint32_t)blocks), dim3(RT_TPB), 0, S, ri, (const uint64_t*)off[t], nrec[t], (uint32_t)t, two ? 2u : 1u, out[t], total[t], dst);
        KCHK(ctx, "k_rows_text");
    }
    ctx->timer.end(S);
    HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    ctx->timer.collect();
    if (hs.err) {
        const unsigned long long wr = hs.bad_row;
        memset(res, 0, sizeof *res);
        if (hs.err & RT_ERR_NAMELB) return rfq_fail(ctx, RFQ_E_DATA, "a line break inside a name (first such row: %llu)", wr);
        if (hs.err & RT_ERR_CODE) return rfq_fail(ctx, RFQ_E_DATA, "a base code above 4 (first such row: %llu)", wr);
        if (hs.err & RT_ERR_BASE) return rfq_fail(ctx, RFQ_E_DATA, "a base outside 0x21..0x7E (first such row: %llu)", wr);
        return rfq_fail(ctx, RFQ_E_DATA, "a quality character outside 0x21..0x7E after the offset %u (first such row: %llu)", (unsigned)in->qual_offset, wr);
    }
    res->d_fq1 = total[0] ? out[0] : nullptr; res->d_fq2 = (two && total[1]) ? out[1] : nullptr;
    return RFQ_OK;
}
extern "C" int rfq_rows_to_text(rfq_ctx* ctx, const rfq_rows_in* in, int32_t paired, uint8_t* d_out1, size_t cap1, uint8_t* d_out2, size_t cap2, int32_t size_only,
        rfq_rows_text_result* res) {
    if (!ctx || !in || !res) return RFQ_E_ARG;
    ctx->err.clear();
    return rows_text_impl(ctx, in, paired, d_out1, cap1, d_out2, cap2, size_only != 0, res);
}
extern "C" int rfq_encode_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_encode_args* enc, rfq_encode_result* res) {
    if (!ctx || !in || !enc || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (enc->d_fq1 || enc->d_fq2 || enc->n1 || enc->n2) return rfq_fail(ctx, RFQ_E_ARG, "rfq_encode_rows fills in the text: d_fq1 / d_fq2 / n1 / n2 must be NULL / 0");
    if (!enc->final && !enc->flush_all) return rfq_fail(ctx, RFQ_E_ARG, "a rows batch is encoded whole: set final or flush_all");
    rfq_rows_text_result t;
    int rc = rows_text_impl(ctx, in, enc->paired, nullptr, 0, nullptr, 0, false, &t);
    if (rc != RFQ_OK) return rc;
    StageSums sums; sums.add(ctx->timer); ctx->timer.names.clear(); ctx->timer.ms.clear();
    rfq_encode_args a = *enc;
    a.d_fq1 = t.d_fq1; a.n1 = t.n1; a.d_fq2 = t.d_fq2; a.n2 = t.n2;
    rc = encode_or_scan(ctx, &a, res, false);
    sums.add(ctx->timer); sums.publish(ctx->timer);                         // the rows stages, then the encoder's own (add merges by name: the two sets of names stay disjoint)
    return rc;
}
// ---------------------------------------------------------------- FASTQ text -> rows, lengths, names: rfq_text_rows of include/rfq_hip.h
// The encoder's own front end - EncBatch, enc_index (without the lazy guess: the totals are needed on the host anyway), normalize_stream on RFQ_NEED_NORM exactly as
// encode_one does - then the sizes kernel, ONE scan of the name sizes and ONE read-back (totals, maxima, error bits, the first bad row, the first empty line, where the
// rows end in each stream); the host decides and launches the writers.  An empty line on normalised text is where the reader stops for good: the sizes pass runs once
// more over the rows in front of it.
struct TextRowsAttempt { uint64_t n_rows, n_bases, names_len; uint32_t max_len, max_name; size_t consumed[2]; bool ended; };
static int text_rows_impl(rfq_ctx* ctx, const rfq_text_rows_args* a, const rfq_encode_args* ea, const NormMap* nm, const uint32_t* skip, bool size_query, TextRowsAttempt* out) {
    hipStream_t S = ctx->stream; DBuf* B = ctx->b; int rc;
    EncBatch b = {}; EncCut cut = {};
    b.a = ea; b.nm = nm; b.skip = skip; b.unit_cap = ~0u; b.fin = ea->final != 0; b.is_pe = ea->paired != RFQ_SE;
    const int nstreams = b.nstreams = ea->paired == RFQ_PE_TWO_FILES ? 2 : 1;
    b.fq[0] = ea->d_fq1; b.fq[1] = nstreams == 2 ? ea->d_fq2 : nullptr;
    b.nbytes[0] = ea->n1 > skip[0] ? ea->n1 : 0; b.nbytes[1] = nstreams == 2 ? (ea->n2 > skip[1] ? ea->n2 : 0) : 0;
    for (int s = 0; s < nstreams; s++) {                                    // (encode_impl's guards: the caller's slice keeps a stream below 4 GiB, the index cannot go without it)
        if (b.nbytes[s] >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "a FASTQ stream of one call must be < 4 GiB (got %zu bytes)", b.nbytes[s]);
        if (b.nbytes[s] && !b.fq[s]) return rfq_fail(ctx, RFQ_E_ARG, "null FASTQ pointer");
        if (b.nbytes[s] && (((uintptr_t)b.fq[s]) & 15u)) return rfq_fail(ctx, RFQ_E_HIP, "internal: FASTQ stream not rounded down to 16 bytes");
    }
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    // (a marker, not a phase: the text has '\r' line ends or blank lines and was rewritten by the normaliser - tests look for it)
    if (nm) { ctx->timer.begin("normalise", S); ctx->timer.end(S); }
    HIPCHK(ctx, table(ctx->d_status, sizeof(DevStatus), b.dst));
    HIPCHK(ctx, fresh_status(ctx, b));
    ctx->lazy_block = true;                                                 // (enc_index takes the flag down again: this index reads its totals back)
    if ((rc = enc_index(ctx, b, cut)) != RFQ_OK) return rc;
    uint32_t n_units = ea->paired == RFQ_SE ? cut.nrec[0] : (ea->paired == RFQ_PE_TWO_FILES ? std::min(cut.nrec[0], cut.nrec[1]) : cut.nrec[0] / 2);
    memset(out, 0, sizeof *out);
    TextRowsStat hs; memset(&hs, 0, sizeof hs); uint64_t names_len = 0; uint32_t cons[2] = { 0, 0 };
    TextRowsStat* dst = nullptr;
    int32_t* lens = nullptr; uint64_t* off = nullptr;
    for (;;) {
        const uint32_t n_rows = n_units * b.T.upr; b.T.n_reads = n_rows;
        if (n_rows == 0) break;
        ctx->timer.begin("text_rows:sizes", S);
        HIPCHK(ctx, table(B[B_LEN], ((size_t)n_rows + 2) * 4, lens)); HIPCHK(ctx, table(B[B_P], ((size_t)n_rows + 2) * 8, off));
        HIPCHK(ctx, B[B_SCANTMP].ensure(std::max<size_t>(1024, ((size_t)n_rows / SCAN_TILE + 2) * 16)));
        if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
        hipLaunchKernelGGL(k_text_rows_sizes, dim3((n_rows + TS_ROWS - 1u) / TS_ROWS), dim3(256), 0, S, b.T, n_rows, lens, off, dst);
        KCHK(ctx, "k_text_rows_sizes");
        scan_exclusive<uint64_t>(S, off, off, n_rows, B[B_SCANTMP].as<uint64_t>(), 1);
        KCHK(ctx, "scan_exclusive");
        ctx->timer.end(S);
        HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
        HIPCHK(ctx, ctx->fetch(&names_len, off + n_rows, 8, S));
        for (int s = 0; s < nstreams; s++) {                                // where the rows end in each stream (enc_verdict's rule)
            const uint32_t recs = ea->paired == RFQ_PE_TWO_FILES ? n_units : n_rows;
            if (nm) HIPCHK(ctx, ctx->fetch(&cons[s], nm->onx[s] + 4 * (size_t)recs - 1, 4, S));
            else HIPCHK(ctx, ctx->fetch(&cons[s], b.T.lo[s] + 4 * (size_t)recs, 4, S));
        }
        HIPCHK(ctx, ctx->fetch_sync(S));
        if (!(hs.err & TR_ERR_EMPTY)) break;
        // "\n\n" is a swallowed blank line, not an empty one: classify the text properly first.  On normalised text an empty line is where
        // FastqReader::read returns NULL (src/fastqreader.cpp:180-191): the record and everything after it are never read.
        if (!nm) return RFQ_NEED_NORM;
        n_units = hs.first_empty / b.T.upr; out->ended = true;
        memset(&hs, 0, sizeof hs); names_len = 0; cons[0] = cons[1] = 0;
    }
    const uint64_t n_rows = (uint64_t)n_units * b.T.upr;
    if (hs.err & TR_ERR_QSHORT) return rfq_fail(ctx, RFQ_E_UNPINNED, "a quality line is shorter than its sequence line (the reference reads past the string: undefined)");
    out->n_rows = n_rows; out->n_bases = hs.n_bases; out->names_len = names_len; out->max_len = hs.max_len; out->max_name = hs.max_name;
    for (int s = 0; s < nstreams; s++) out->consumed[s] = n_rows ? (size_t)consumed_of(b, s, cons[s]) : 0;
    if (size_query) { ctx->timer.collect(); return RFQ_OK; }
    if ((rc = rows_room(ctx, a, n_rows, names_len, hs.max_len)) != RFQ_OK) return rc;
    if (n_rows == 0) return rows_none(ctx, a->d_name_off);
    ctx->timer.begin("text_rows:rows", S);
    if (a->d_lens) HIPCHK(ctx, hipMemcpyAsync(a->d_lens, lens, (size_t)n_rows * 4, hipMemcpyDeviceToDevice, S));
    if (a->d_bases || a->d_quals) {
        TextRowsOut o; memset(&o, 0, sizeof o);
        o.bases = a->d_bases; o.quals = a->d_quals; o.row_len = a->row_len; o.n_rows = (uint32_t)n_rows; o.codes = a->base_mode == RFQ_ROWS_CODE ? 1u : 0u;
        o.qoff4 = a->qual_offset * 0x01010101u; o.pad_b4 = a->pad_base * 0x01010101u; o.pad_q4 = a->pad_qual * 0x01010101u;
        o.vec = rows_vec(a->row_len, a->d_bases, a->d_quals); o.per = rows_per(a->row_len);
        hipLaunchKernelGGL(k_text_rows, dim3((uint32_t)((n_rows + o.per - 1) / o.per)), dim3(256), 0, S, b.T, o, dst);
        KCHK(ctx, "k_text_rows");
    }
    ctx->timer.end(S);
    ctx->timer.begin("text_rows:names", S);
    if (a->d_name_off) HIPCHK(ctx, hipMemcpyAsync(a->d_name_off, off, (size_t)(n_rows + 1) * 8, hipMemcpyDeviceToDevice, S));
    if (a->d_names && names_len) {
        uint32_t blocks = 0;
        if ((rc = name_blob_blocks(ctx, a->d_names, names_len, &blocks)) != RFQ_OK) return rc;
        hipLaunchKernelGGL(k_text_names, dim3(blocks), dim3(TN_TPB), 0, S, b.T, (const uint64_t*)off, (uint32_t)n_rows, a->d_names, names_len);
        KCHK(ctx, "k_text_names");
    }
    ctx->timer.end(S);
    HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    ctx->timer.collect();
    if (hs.err & TR_ERR_BASE) return rfq_fail(ctx, RFQ_E_DATA, "a base that is not one of A C G T N cannot be a code (first such row: %llu)", (unsigned long long)hs.bad_row);
    return RFQ_OK;
}
extern "C" int rfq_text_rows(rfq_ctx* ctx, const rfq_text_rows_args* a, rfq_text_rows_result* res) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (a->paired < 0 || a->paired > 2) return rfq_fail(ctx, RFQ_E_ARG, "paired must be RFQ_SE, RFQ_PE_TWO_FILES or RFQ_PE_INTERLEAVED");
    const bool two = a->paired == RFQ_PE_TWO_FILES;
    if (!two && a->d_fq2) return rfq_fail(ctx, RFQ_E_ARG, "d_fq2 is for RFQ_PE_TWO_FILES");
    const bool size_query = !a->d_bases && !a->d_quals && !a->d_lens && !a->d_names && !a->d_name_off;
    if (!size_query && a->row_len == 0) return rfq_fail(ctx, RFQ_E_ARG, "row_len must be >= 1");
    if (a->base_mode != RFQ_ROWS_ASCII && a->base_mode != RFQ_ROWS_CODE) return rfq_fail(ctx, RFQ_E_ARG, "base_mode must be RFQ_ROWS_ASCII or RFQ_ROWS_CODE");
    if (((uintptr_t)a->d_lens & 3u) || ((uintptr_t)a->d_name_off & 7u)) return rfq_fail(ctx, RFQ_E_ARG, "d_lens must be 4-byte and d_name_off 8-byte aligned");
    // One call indexes with 32-bit offsets: of each stream at most the encoder's slice; what lies beyond it is the next call's (this one is then not final)
    size_t slice, lim; slice_limits(ctx, slice, lim);
    rfq_encode_args ea; memset(&ea, 0, sizeof ea);
    ea.paired = a->paired; ea.chunk_bases = 1; ea.final = a->final ? 1 : 0;
    ea.d_fq1 = a->d_fq1; ea.n1 = a->n1; ea.file_off1 = a->file_off1;
    if (two) { ea.d_fq2 = a->d_fq2; ea.n2 = a->n2; ea.file_off2 = a->file_off2; }
    if (ea.n1 >= lim) { ea.n1 = slice; ea.final = 0; }
    if (two && ea.n2 >= lim) { ea.n2 = slice; ea.final = 0; }
    rfq_encode_args al; uint32_t skip[2];
    align_streams(&ea, al, skip);
    TextRowsAttempt t;
    int rc = text_rows_impl(ctx, a, &al, nullptr, skip, size_query, &t);
    if (rc == RFQ_NEED_NORM) {
        NormMap nm; rfq_encode_args a2; const uint32_t noskip[2] = { 0, 0 };
        if ((rc = normalize_streams(ctx, &ea, a2, nm)) != RFQ_OK) return rc;
        rc = text_rows_impl(ctx, a, &a2, &nm, noskip, size_query, &t);
        if (rc == RFQ_NEED_NORM) return rfq_fail(ctx, RFQ_E_HIP, "internal: normalised text still needs normalisation");
    }
    if (rc != RFQ_OK) return rc;
    res->n_rows = t.n_rows; res->n_bases = t.n_bases; res->names_len = t.names_len; res->max_len = t.max_len; res->max_name = t.max_name;
    res->consumed1 = t.consumed[0]; res->consumed2 = two ? t.consumed[1] : 0; res->input_ended = t.ended ? 1 : 0;
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows -> kept, trimmed rows with their names: rfq_select_rows of include/rfq_hip.h
// A compacting call over ROWS (the plan: rows_judge / rows_write above).  The judging pass (k_sel_judge), TWO scans - the kept flags to output row indices (32-bit),
// the kept name sizes to output name offsets (64-bit: a blob may exceed 4 GiB, and the block scan's wave primitives take 4- and 8-byte values, not a two-field
// struct) - and ONE read-back: the verdict block and the two totals.  The host refuses or goes on; k_sel_tables makes the per-output-row tables (and the caller's
// lens / name_off), k_sel_rows and k_sel_names follow them.
static const RowsStages SELECT_STAGES = { "select:judge", "select:tables", "select:rows", "select:names" };
// ---- rfq_select_rows with a tag (rfq_name_tag; enc/rows_tag.h).  What the host judges of it:
#define TAG_X_MAX (1ull + RFQ_TAG_PREFIX_MAX + 1ull + 2ull * RFQ_TAG_PART_MAX + 1ull)        // sep, prefix, join, two parts and the join between them: 81
static int select_tag_arg(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_name_tag* t, bool named) {
    auto graph = [](uint8_t c) { return c >= 0x21u && c <= 0x7Eu; };
    int rc;
    if (!named) return rfq_fail(ctx, RFQ_E_ARG, "rows without names (d_name_off == NULL) take no tag");
    if (in->n_rows && (!t->d_tag_start || !t->d_tag_len)) return rfq_fail(ctx, RFQ_E_ARG, "tag: null d_tag_start / d_tag_len");
    if (((uintptr_t)t->d_tag_start | (uintptr_t)t->d_tag_len) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "tag: d_tag_start and d_tag_len must be 4-byte aligned");
    if (t->prefix_len > RFQ_TAG_PREFIX_MAX) return rfq_fail(ctx, RFQ_E_ARG, "tag: prefix_len is at most %d (got %u)", RFQ_TAG_PREFIX_MAX, t->prefix_len);
    if (t->prefix_len && !t->h_prefix) return rfq_fail(ctx, RFQ_E_ARG, "tag: null h_prefix with prefix_len = %u", t->prefix_len);
    if (!graph(t->sep) || !graph(t->join)) return rfq_fail(ctx, RFQ_E_ARG, "tag: sep and join must be bytes in 0x21..0x7E (got 0x%02x, 0x%02x)", t->sep, t->join);
    for (uint32_t i = 0; i < t->prefix_len; i++)
        if (!graph(t->h_prefix[i])) return rfq_fail(ctx, RFQ_E_ARG, "tag: the prefix holds a byte outside 0x21..0x7E (0x%02x at %u)", t->h_prefix[i], i);
    if (t->at != RFQ_TAG_AT_SPACE && t->at != RFQ_TAG_AT_END) return rfq_fail(ctx, RFQ_E_ARG, "tag: at must be RFQ_TAG_AT_SPACE or RFQ_TAG_AT_END (got %u)", t->at);
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if (in->n_rows && !in->d_bases) return rfq_fail(ctx, RFQ_E_ARG, "tag: null rows->d_bases");
    return RFQ_OK;
}
// The names step of such a call: the plan (select:tagplan) and the writer that follows it, or - RFQ_TAG=general - the byte-wise writer alone (select:names either way)
static int select_names_tag(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_select_rows_args* a, const RowsJudged& j, const TagIn& ti, const SelRow* tab, const uint64_t* ooff) {
    hipStream_t S = ctx->stream; int rc;
    const bool wanted = a->d_names && j.names_len, general = ctx->opt.tag_general;
    TagNames nm; memset(&nm, 0, sizeof nm);
    nm.names = in->d_names; nm.in_off = in->d_name_off; nm.names_len = in->names_len; nm.tab = tab; nm.n_out = j.n_out;
    uint8_t* xs = nullptr;
    if (wanted && !general) {
        ctx->timer.begin("select:tagplan", S);
        HIPCHK(ctx, table(ctx->tag_x, (size_t)j.n_out * TAG_STRIDE, xs));
        hipLaunchKernelGGL(k_tag_plan, dim3((uint32_t)(((uint64_t)j.n_out + TP_ROWS - 1u) / TP_ROWS)), dim3(256), 0, S, ti, nm, xs);
        KCHK(ctx, "k_tag_plan");
        ctx->timer.end(S);
    }
    ctx->timer.begin(SELECT_STAGES.names, S);
    if (wanted && general) {
        hipLaunchKernelGGL(k_sel_names_tag_general, dim3((uint32_t)(((uint64_t)j.n_out + 255u) / 256u)), dim3(256), 0, S, ti, nm, ooff, a->d_names);
        KCHK(ctx, "k_sel_names_tag_general");
    } else if (wanted) {
        uint32_t blocks = 0;
        if ((rc = name_blob_blocks(ctx, a->d_names, j.names_len, &blocks)) != RFQ_OK) return rc;
        hipLaunchKernelGGL(k_sel_names_tag, dim3(blocks), dim3(TN_TPB), 0, S, nm, (const uint8_t*)xs, ooff, a->d_names, j.names_len);
        KCHK(ctx, "k_sel_names_tag");
    }
    ctx->timer.end(S);
    return RFQ_OK;
}
extern "C" int rfq_select_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_select_rows_args* a, rfq_select_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows; const bool named = in->d_name_off != nullptr;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    if ((rc = rows_dst_len(ctx, a)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, true)) != RFQ_OK) return rc;
    if (n >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if ((rc = rows_dst_named(ctx, a, named)) != RFQ_OK) return rc;
    if (n && (!in->d_lens || (a->d_bases && !in->d_bases) || (a->d_quals && !in->d_quals) || (a->d_names && in->names_len && !in->d_names)))
        return rfq_fail(ctx, RFQ_E_ARG, "null row / name pointer");
    if ((rc = rows_dst_aligned(ctx, in, a, (uintptr_t)a->d_start | (uintptr_t)a->d_len, "d_lens, d_start and d_len")) != RFQ_OK) return rc;
    const rfq_name_tag* const tg = a->tag;
    if (tg && (rc = select_tag_arg(ctx, in, tg, named)) != RFQ_OK) return rc;
    {   // the bytes a call can write (its cap, and never more than n_rows rows of row_len) against the bytes it reads; with a tag the names grow by up to TAG_X_MAX each
        Span ins[10]; rows_src_spans(in, named, ins);
        ins[5] = { a->d_keep, n, "d_keep" }; ins[6] = { a->d_start, n * 4ull, "d_start" }; ins[7] = { a->d_len, n * 4ull, "d_len" };
        ins[8] = { tg ? tg->d_tag_start : nullptr, n * 4ull, "tag->d_tag_start" }; ins[9] = { tg ? tg->d_tag_len : nullptr, n * 4ull, "tag->d_tag_len" };
        Span outs[5]; rows_dst_spans(a, n, (uint64_t)in->names_len + (tg ? n * TAG_X_MAX : 0ull), outs);
        if ((rc = rows_apart(ctx, outs, ins, ": selection in place is not offered")) != RFQ_OK) return rc;
    }
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    res->n_in = n;
    SelIn si; memset(&si, 0, sizeof si);
    si.lens = in->d_lens; si.name_off = in->d_name_off; si.keep = a->d_keep; si.start = a->d_start; si.len = a->d_len;
    si.names_len = in->names_len; si.n_rows = (uint32_t)n; si.row_len = in->row_len; si.pairs = a->pairs ? 1u : 0u; si.min_len = a->min_len;
    TagIn ti; memset(&ti, 0, sizeof ti);
    if (tg) {
        ti.tstart = tg->d_tag_start; ti.tlen = tg->d_tag_len; ti.lens = in->d_lens; ti.bases = in->d_bases; ti.total = n * in->row_len; ti.row_len = in->row_len;
        ti.codes = in->base_mode == RFQ_ROWS_CODE ? 1u : 0u; ti.pairs = si.pairs; ti.prefix_len = tg->prefix_len; ti.sep = tg->sep; ti.join = tg->join; ti.at = tg->at;
        if (tg->prefix_len) memcpy(ti.prefix, tg->h_prefix, tg->prefix_len);
    }
    SelStat hs; RowsJudged j;
    rc = rows_judge(ctx, n, named, SELECT_STAGES.judge, [&](uint32_t* flag, uint64_t* nsz, SelStat* dst) -> int {
        const dim3 grid((uint32_t)((n + SJ_ROWS - 1u) / SJ_ROWS));
        if (tg) { hipLaunchKernelGGL(k_sel_judge_tag, grid, dim3(256), 0, ctx->stream, si, ti, flag, nsz, dst); return launched(ctx, "k_sel_judge_tag"); }
        hipLaunchKernelGGL(k_sel_judge, grid, dim3(256), 0, ctx->stream, si, flag, nsz, dst);
        return launched(ctx, "k_sel_judge");
    }, &hs, &j);
    if (rc != RFQ_OK) return rc;
    const unsigned long long br = hs.bad_row;
    if (hs.err & SL_ERR_LEN) return rows_len_refusal(ctx, in->row_len, br);
    if (hs.err & SL_ERR_WIN) return rfq_fail(ctx, RFQ_E_ARG, "a window starts below 0, has a negative length or ends behind its read (first such row: %llu)", br);
    if (hs.err & SL_ERR_NOFF) return rfq_fail(ctx, RFQ_E_ARG, "the name offsets decrease or end past names_len = %zu (first such row: %llu)", in->names_len, br);
    if (hs.err & SL_ERR_TAG) return rfq_fail(ctx, RFQ_E_ARG, "a tag part starts below 0, has a negative length, more than %d bases or ends behind its read (first such row: %llu)", RFQ_TAG_PART_MAX, br);
    if (hs.err & SL_ERR_TAGB) return rfq_fail(ctx, RFQ_E_DATA, "a tag part holds %s (first such row: %llu)", ti.codes ? "a base code above 4" : "a byte outside 0x21..0x7E", br);
    if (tg && hs.max_name == 0xFFFFFFFFu) return rfq_fail(ctx, RFQ_E_ARG, "a name of 4 GiB or more takes no tag");
    res->n_rows = j.n_out; res->n_bases = hs.n_bases; res->names_len = j.names_len; res->max_len = hs.max_len; res->max_name = hs.max_name;
    res->dropped_mask = hs.d_mask; res->dropped_short = hs.d_short; res->dropped_mate = hs.d_mate;
    if (rows_size_query(a)) { ctx->timer.collect(); return RFQ_OK; }
    if ((rc = rows_room(ctx, a, j.n_out, j.names_len, hs.max_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    if (j.n_out == 0) return rows_none(ctx, a->d_name_off);
    auto tables = [&](const uint32_t* pos, const uint64_t* noff, SelRow* tab, uint64_t* ooff) -> int {
        hipLaunchKernelGGL(k_sel_tables, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, ctx->stream, si, pos, noff, tab, ooff, a->d_lens, a->d_name_off);
        return launched(ctx, "k_sel_tables");
    };
    auto rows = [&](RowsOut& r, const SelRow* tab) -> int {
        r.vec_in = rows_vec(in->row_len, a->d_bases ? in->d_bases : nullptr, a->d_quals ? in->d_quals : nullptr);      // (of the buffers that are read)
        hipLaunchKernelGGL(k_sel_rows, dim3((uint32_t)(((uint64_t)r.n_out + r.per - 1) / r.per)), dim3(256), 0, ctx->stream, r, tab);
        return launched(ctx, "k_sel_rows");
    };
    if (!tg) return rows_write(ctx, in, a, j, SELECT_STAGES, tables, rows);
    return rows_write(ctx, in, a, j, SELECT_STAGES, tables, rows, [&](const SelRow* tab, const uint64_t* ooff) -> int { return select_names_tag(ctx, in, a, j, ti, tab, ooff); });
}
// ---------------------------------------------------------------- rows -> the kept rows grouped by a bin per unit, in one pass: rfq_group_rows of include/rfq_hip.h
// rfq_select_rows with another ordering step (enc/rows_group.h).  The judging pass is select's under one more rule (k_group_judge) and leaves a word per unit and
// every sum a size query answers - nothing is scanned in input order -, k_group_used counts the bins that hold a row: ONE read-back.  The host refuses or goes on:
// the stable rank (group_rank: one or two passes of histogram, scan, scatter), then rows_write with tables made in OUTPUT order and select's two writers as they are.
static const RowsStages GROUP_STAGES = { "group:judge", "group:tables", "group:rows", "group:names" };
// The kept units sorted by (key, unit), stable: *skey / *sidx [units_out].  One pass of 8-bit digits up to 256 bins, two beyond; the first reads the judge's words.
static int group_rank(rfq_ctx* ctx, const uint32_t* kk, uint32_t units, uint32_t units_out, uint32_t T, const uint16_t** skey, const uint32_t** sidx) {
    hipStream_t S = ctx->stream;
    const int passes = T > 256u ? 2 : 1;
    for (int p = 0; p < passes; p++) { HIPCHK(ctx, ctx->group_key[p].ensure((size_t)units_out * 2 + 16)); HIPCHK(ctx, ctx->group_idx[p].ensure((size_t)units_out * 4 + 16)); }
    const uint32_t tiles0 = (uint32_t)(((uint64_t)units + GR_TILE - 1) / GR_TILE);
    const uint64_t cells0 = 256ull * tiles0;
    HIPCHK(ctx, ctx->group_hist.ensure((size_t)(cells0 + 2) * 4));
    // (the scans' scratch once, for the digit table here and for the name sizes of the output rows behind this: growing it later would wait for the device)
    HIPCHK(ctx, ctx->b[B_SCANTMP].ensure(std::max<size_t>(1024, ((size_t)std::max<uint64_t>(cells0, 2ull * units_out) / SCAN_TILE + 2) * 16)));
    uint32_t* hist = ctx->group_hist.as<uint32_t>();
    for (int p = 0; p < passes; p++) {
        GrSrc s; memset(&s, 0, sizeof s);
        if (p == 0) { s.kk = kk; s.n = units; } else { s.key = ctx->group_key[0].as<uint16_t>(); s.idx = ctx->group_idx[0].as<uint32_t>(); s.n = units_out; }
        s.shift = 8u * (uint32_t)p;
        const uint32_t tiles = (uint32_t)(((uint64_t)s.n + GR_TILE - 1) / GR_TILE);
        hipLaunchKernelGGL(k_gr_hist, dim3(tiles), dim3(256), 0, S, s, tiles, hist);
        KCHK(ctx, "k_gr_hist");
        scan_exclusive<uint32_t>(S, hist, hist, 256ull * tiles, ctx->b[B_SCANTMP].as<uint32_t>(), 0);
        KCHK(ctx, "scan_exclusive");
        hipLaunchKernelGGL(k_gr_scatter, dim3(tiles), dim3(256), 0, S, s, tiles, (const uint32_t*)hist, ctx->group_key[p].as<uint16_t>(), ctx->group_idx[p].as<uint32_t>());
        KCHK(ctx, "k_gr_scatter");
    }
    *skey = ctx->group_key[passes - 1].as<uint16_t>(); *sidx = ctx->group_idx[passes - 1].as<uint32_t>();
    return RFQ_OK;
}
extern "C" int rfq_group_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_group_rows_args* a, rfq_group_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows; const bool named = in->d_name_off != nullptr;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    const bool rows_asked = !rows_size_query(a), size_query = !rows_asked && !a->d_bin_off;      // (the five outputs of select; all six)
    if ((rc = rows_dst_len(ctx, a)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, true)) != RFQ_OK) return rc;
    if (n >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if ((rc = rows_dst_named(ctx, a, named)) != RFQ_OK) return rc;
    if (n && (!in->d_lens || (a->d_bases && !in->d_bases) || (a->d_quals && !in->d_quals) || (a->d_names && in->names_len && !in->d_names)))
        return rfq_fail(ctx, RFQ_E_ARG, "null row / name pointer");
    if (n && !a->d_bin) return rfq_fail(ctx, RFQ_E_ARG, "null d_bin");
    if (a->n_bins == 0) return rfq_fail(ctx, RFQ_E_ARG, "n_bins must be >= 1");
    if (a->rest != 0 && a->rest != 1) return rfq_fail(ctx, RFQ_E_ARG, "rest must be 0 or 1");
    const uint64_t T64 = (uint64_t)a->n_bins + (uint64_t)a->rest;
    if (T64 > GR_MAX_BINS) return rfq_fail(ctx, RFQ_E_ARG, "n_bins + rest is at most %u (got %llu)", GR_MAX_BINS, (unsigned long long)T64);
    const uint32_t T = (uint32_t)T64, nr = a->pairs ? 2u : 1u;
    const uint64_t units = n / nr;
    if ((rc = rows_dst_aligned(ctx, in, a, (uintptr_t)a->d_start | (uintptr_t)a->d_len | (uintptr_t)a->d_bin, "d_lens, d_start, d_len and d_bin")) != RFQ_OK) return rc;
    if ((uintptr_t)a->d_bin_off & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_bin_off must be 8-byte aligned");
    {   // the bytes a call can write against the bytes it reads: select's spans, with d_bin among the inputs and d_bin_off among the outputs
        Span ins[9]; rows_src_spans(in, named, ins);
        ins[5] = { a->d_keep, n, "d_keep" }; ins[6] = { a->d_start, n * 4ull, "d_start" }; ins[7] = { a->d_len, n * 4ull, "d_len" }; ins[8] = { a->d_bin, units * 4ull, "d_bin" };
        Span five[5]; rows_dst_spans(a, n, in->names_len, five);
        Span outs[6]; for (int i = 0; i < 5; i++) outs[i] = five[i];
        outs[5] = { a->d_bin_off, std::min<unsigned long long>(a->bin_cap, T64 + 1) * 8ull, "d_bin_off" };
        if ((rc = rows_apart(ctx, outs, ins, ": grouping in place is not offered")) != RFQ_OK) return rc;
    }
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    hipStream_t S = ctx->stream;
    res->n_in = n;
    SelIn si; memset(&si, 0, sizeof si);
    si.lens = in->d_lens; si.name_off = in->d_name_off; si.keep = a->d_keep; si.start = a->d_start; si.len = a->d_len;
    si.names_len = in->names_len; si.n_rows = (uint32_t)n; si.row_len = in->row_len; si.pairs = a->pairs ? 1u : 0u; si.min_len = a->min_len;
    GroupStat hs; memset(&hs, 0, sizeof hs);
    uint32_t* kk = nullptr;
    if (n) {
        ctx->timer.begin(GROUP_STAGES.judge, S);
        GroupIn gi; memset(&gi, 0, sizeof gi);
        gi.bin = a->d_bin; gi.n_bins = a->n_bins; gi.rest = (uint32_t)a->rest; gi.words = (T + 31u) / 32u;
        HIPCHK(ctx, table(ctx->group_kk, (size_t)units * 4 + 16, kk));
        HIPCHK(ctx, table(ctx->group_used, (size_t)GR_MAX_BINS / 8, gi.used));
        HIPCHK(ctx, hipMemsetAsync(gi.used, 0, (size_t)gi.words * 4, S));
        gi.kk = kk;
        GroupStat* dst = nullptr;
        if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
        hipLaunchKernelGGL(k_group_judge, dim3((uint32_t)((n + SJ_ROWS - 1u) / SJ_ROWS)), dim3(256), 0, S, si, gi, dst);
        KCHK(ctx, "k_group_judge");
        hipLaunchKernelGGL(k_group_used, dim3(1), dim3(256), 0, S, (const uint32_t*)gi.used, gi.words, dst);
        KCHK(ctx, "k_group_used");
        ctx->timer.end(S);
        HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
        HIPCHK(ctx, ctx->fetch_sync(S));
    }
    const unsigned long long br = hs.bad_row;
    if (hs.err & SL_ERR_LEN) return rows_len_refusal(ctx, in->row_len, br);
    if (hs.err & SL_ERR_WIN) return rfq_fail(ctx, RFQ_E_ARG, "a window starts below 0, has a negative length or ends behind its read (first such row: %llu)", br);
    if (hs.err & SL_ERR_NOFF) return rfq_fail(ctx, RFQ_E_ARG, "the name offsets decrease or end past names_len = %zu (first such row: %llu)", in->names_len, br);
    if (hs.err & GR_ERR_BIN) return rfq_fail(ctx, RFQ_E_ARG, "a bin is not below n_bins = %u (first such unit: %llu)", a->n_bins, (unsigned long long)hs.bad_unit);
    const uint32_t n_out = (uint32_t)hs.n_kept;
    res->n_rows = n_out; res->n_bases = hs.n_bases; res->names_len = hs.names_len; res->max_len = hs.max_len; res->max_name = hs.max_name;
    res->dropped_mask = hs.d_mask; res->dropped_short = hs.d_short; res->dropped_mate = hs.d_mate; res->dropped_bin = hs.d_bin; res->n_bins_used = hs.n_used;
    if (size_query) { ctx->timer.collect(); return RFQ_OK; }
    if (a->d_bin_off && a->bin_cap < T64 + 1) {
        memset(res, 0, sizeof *res);
        return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffers too small: need %llu bin offsets (bin_cap < T + 1 = n_bins + rest + 1)", (unsigned long long)(T64 + 1));
    }
    if (rows_asked && (rc = rows_room(ctx, a, n_out, hs.names_len, hs.max_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    if (n_out == 0) {
        if (a->d_bin_off) HIPCHK(ctx, hipMemsetAsync(a->d_bin_off, 0, (size_t)(T + 1) * 8, S));
        return rows_none(ctx, a->d_name_off);
    }
    const uint32_t units_out = n_out / nr;
    const uint16_t* skey = nullptr; const uint32_t* sidx = nullptr;
    ctx->timer.begin("group:rank", S);
    if ((rc = group_rank(ctx, kk, (uint32_t)units, units_out, T, &skey, &sidx)) != RFQ_OK) return rc;
    ctx->timer.end(S);
    RowsJudged j; j.n_out = n_out; j.names_len = hs.names_len;
    if (named) HIPCHK(ctx, table(ctx->b[B_P], ((size_t)n_out + 2) * 8, j.noff));          // (the name sizes in output order, scanned into rows_write's offsets)
    return rows_write(ctx, in, a, j, GROUP_STAGES,
        [&](const uint32_t*, const uint64_t* nsz, SelRow* tab, uint64_t* ooff) -> int {
            hipLaunchKernelGGL(k_group_tables, dim3((units_out + 255u) / 256u), dim3(256), 0, S, si, sidx, units_out, tab, (uint64_t*)nsz, a->d_lens);
            KCHK(ctx, "k_group_tables");
            if (named) {
                scan_exclusive<uint64_t>(S, nsz, ooff, n_out, ctx->b[B_SCANTMP].as<uint64_t>(), 1);
                KCHK(ctx, "scan_exclusive");
                if (a->d_name_off) HIPCHK(ctx, hipMemcpyAsync(a->d_name_off, ooff, ((size_t)n_out + 1) * 8, hipMemcpyDeviceToDevice, S));
            }
            if (a->d_bin_off) {
                hipLaunchKernelGGL(k_group_bin_off, dim3((T + 256u) / 256u), dim3(256), 0, S, skey, units_out, T, nr, a->d_bin_off);
                KCHK(ctx, "k_group_bin_off");
            }
            return RFQ_OK;
        },
        [&](RowsOut& r, const SelRow* tab) -> int {
            r.vec_in = rows_vec(in->row_len, a->d_bases ? in->d_bases : nullptr, a->d_quals ? in->d_quals : nullptr);      // (of the buffers that are read)
            hipLaunchKernelGGL(k_sel_rows, dim3((uint32_t)(((uint64_t)r.n_out + r.per - 1) / r.per)), dim3(256), 0, S, r, tab);
            return launched(ctx, "k_sel_rows");
        });
}
// ---------------------------------------------------------------- pairs -> one row per overlapping pair, under R1's name: rfq_merge_rows of include/rfq_hip.h
// A compacting call over PAIRS: the judging pass (k_merge_judge), the tables (k_merge_tables), two row writers - k_merge_rows (RFQ_MERGE=general: k_merge_rows_any) -
// and k_sel_names as it is, over a table that keeps the source row where it reads it (enc/rows_merge.h).
static const RowsStages MERGE_STAGES = { "merge:judge", "merge:tables", "merge:rows", "merge:names" };
extern "C" int rfq_merge_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_merge_rows_args* a, rfq_merge_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows, np = n / 2; const bool named = in->d_name_off != nullptr;
    int rc;
    if (n & 1u) return rfq_fail(ctx, RFQ_E_ARG, "merging takes rows in pairs (got %llu rows)", (unsigned long long)n);
    if ((rc = rows_dst_len(ctx, a)) != RFQ_OK) return rc;
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n >= 0xFFFFFFF0ull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if ((rc = rows_dst_named(ctx, a, named)) != RFQ_OK) return rc;
    if (n && !a->d_insert) return rfq_fail(ctx, RFQ_E_ARG, "null d_insert");
    if (n && (!in->d_lens || (a->d_names && in->names_len && !in->d_names))) return rfq_fail(ctx, RFQ_E_ARG, "null row / name pointer");
    if (n && (a->d_bases || a->d_quals) && (!in->d_bases || !in->d_quals))
        return rfq_fail(ctx, RFQ_E_ARG, "a row output needs rows->d_bases and rows->d_quals, both: the rule looks at the bases and the scores");
    if ((rc = rows_dst_aligned(ctx, in, a, (uintptr_t)a->d_insert, "d_lens and d_insert")) != RFQ_OK) return rc;
    {   // the bytes a call can write (its cap, and never more than n_rows / 2 rows of row_len) against the bytes it reads
        Span ins[6]; rows_src_spans(in, named, ins);
        ins[5] = { a->d_insert, np * 4ull, "d_insert" };
        Span outs[5]; rows_dst_spans(a, np, in->names_len, outs);
        if ((rc = rows_apart(ctx, outs, ins, ": merging in place is not offered")) != RFQ_OK) return rc;
    }
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    res->n_pairs = np;
    MergeIn mi; memset(&mi, 0, sizeof mi);
    mi.lens = in->d_lens; mi.insert = a->d_insert; mi.name_off = in->d_name_off; mi.names_len = in->names_len;
    mi.n_rows = (uint32_t)n; mi.n_pairs = (uint32_t)np; mi.row_len = in->row_len;
    MergeStat hs; RowsJudged j;
    rc = rows_judge(ctx, np, named, MERGE_STAGES.judge, [&](uint32_t* flag, uint64_t* nsz, MergeStat* dst) -> int {
        hipLaunchKernelGGL(k_merge_judge, dim3((uint32_t)((np + MJ_PAIRS - 1u) / MJ_PAIRS)), dim3(256), 0, ctx->stream, mi, flag, nsz, dst);
        return launched(ctx, "k_merge_judge");
    }, &hs, &j);
    if (rc != RFQ_OK) return rc;
    if (hs.err) {                                                            // the first offender's key says which rule it broke (enc/rows_merge.h)
        const unsigned long long row = hs.bad_row >> 2;
        switch ((uint32_t)(hs.bad_row & 3u)) {
        case MG_ERR_LEN: return rows_len_refusal(ctx, in->row_len, row);
        case MG_ERR_INS: return rfq_fail(ctx, RFQ_E_ARG, "a pair with insert >= 0 has no position that both mates cover: an empty mate, insert == 0 or insert > l1 + l2 - 1 (first such pair: %llu)", row / 2);
        default: return rfq_fail(ctx, RFQ_E_ARG, "the name offsets decrease or end past names_len = %zu (first such row: %llu)", in->names_len, row);
        }
    }
    res->n_rows = j.n_out; res->n_bases = hs.n_bases; res->names_len = j.names_len; res->max_len = hs.max_len; res->max_name = hs.max_name; res->overlap_bases = hs.overlap;
    if (rows_size_query(a)) { ctx->timer.collect(); return RFQ_OK; }
    if ((rc = rows_room(ctx, a, j.n_out, j.names_len, hs.max_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    if (j.n_out == 0) return rows_none(ctx, a->d_name_off);
    return rows_write(ctx, in, a, j, MERGE_STAGES,
        [&](const uint32_t* pos, const uint64_t* noff, SelRow* tab, uint64_t* ooff) -> int {
            hipLaunchKernelGGL(k_merge_tables, dim3((uint32_t)((np + 255) / 256)), dim3(256), 0, ctx->stream, mi, pos, noff, tab, ooff, a->d_lens, a->d_name_off);
            return launched(ctx, "k_merge_tables");
        },
        [&](RowsOut& r, const SelRow* tab) -> int {
            r.vec_in = rows_vec(in->row_len, in->d_bases, in->d_quals);
            r.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u;
            if (ctx->opt.merge_general) {
                const unsigned long long nb = ((unsigned long long)r.n_out * a->row_len + 255ull) / 256ull;
                if (nb > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "RFQ_MERGE=general: %llu output bytes are too many for one call", (unsigned long long)r.n_out * a->row_len);
                hipLaunchKernelGGL(k_merge_rows_any, dim3((uint32_t)nb), dim3(256), 0, ctx->stream, r, tab);
            } else hipLaunchKernelGGL(k_merge_rows, dim3((uint32_t)(((uint64_t)r.n_out + r.per - 1) / r.per)), dim3(256), 0, ctx->stream, r, tab);
            return launched(ctx, "k_merge_rows");
        });
}
// ---------------------------------------------------------------- rows -> keep, window, reason and metrics per row, one QC summary: rfq_judge_rows of include/rfq_hip.h
// One kernel (rows_launch_by_len; with RFQ_JUDGE=general the wave-per-row kernel in tiles of 64, enc/rows_judge.h) and one read-back (the verdict block with the sums).
extern "C" int rfq_judge_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_judge_rows_args* a, rfq_judge_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if (a->cut_flags & ~(RFQ_CUT_FRONT | RFQ_CUT_RIGHT | RFQ_CUT_TAIL)) return rfq_fail(ctx, RFQ_E_ARG, "unknown cut_flags bits (0x%x)", a->cut_flags);
    if (a->cut_flags && (a->cut_window < 1u || a->cut_window > 1000u)) return rfq_fail(ctx, RFQ_E_ARG, "cut_window must be 1 .. 1000 with a cut flag (got %u)", a->cut_window);
    if (a->max_lowq_pct > 100u || a->min_complexity_pct > 100u) return rfq_fail(ctx, RFQ_E_ARG, "a percentage is 0 .. 100 (max_lowq_pct %u, min_complexity_pct %u)", a->max_lowq_pct, a->min_complexity_pct);
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if (n && !in->d_lens) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens");
    const bool need_q = a->cut_flags || a->min_mean_q || a->qual_q, need_b = a->poly_g || a->max_n >= 0 || a->min_complexity_pct;
    if (n && need_q && !in->d_quals) return rfq_fail(ctx, RFQ_E_ARG, "a quality criterion (a cut flag, min_mean_q, qual_q) needs rows->d_quals");
    if (n && need_b && !in->d_bases) return rfq_fail(ctx, RFQ_E_ARG, "a base criterion (poly_g, max_n, min_complexity_pct) needs rows->d_bases");
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_start | (uintptr_t)a->d_len | (uintptr_t)a->d_metrics) & 3u)
        return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_start, d_len and d_metrics must be 4-byte aligned");
    {
        Span ins[5]; rows_src_spans(in, false, ins);
        const Span outs[] = {
            { a->d_keep, n, "d_keep" }, { a->d_start, n * 4ull, "d_start" }, { a->d_len, n * 4ull, "d_len" }, { a->d_why, n, "d_why" }, { a->d_metrics, n * 16ull, "d_metrics" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
    }
    res->n_rows = n;
    if (!n) return RFQ_OK;
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    JudgeIn ji; memset(&ji, 0, sizeof ji);
    ji.b = in->d_bases; ji.q = in->d_quals; ji.lens = in->d_lens; ji.total = n * in->row_len; ji.n_rows = (uint32_t)n; ji.row_len = in->row_len;
    ji.vec_in = rows_vec(in->row_len, in->d_bases, in->d_quals);
    ji.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u;
    ji.trim_front = a->trim_front; ji.trim_tail = a->trim_tail; ji.poly_g = a->poly_g; ji.cut_flags = a->cut_flags; ji.cut_window = a->cut_window; ji.cut_mean_q = a->cut_mean_q;
    ji.max_len = a->max_len; ji.min_len = a->min_len; ji.max_n = a->max_n; ji.min_mean_q = a->min_mean_q; ji.qual_q = a->qual_q; ji.max_lowq_pct = a->max_lowq_pct;
    ji.min_complexity_pct = a->min_complexity_pct;
    ji.keep = a->d_keep; ji.start = a->d_start; ji.len = a->d_len; ji.why = a->d_why; ji.metrics = a->d_metrics;
    ji.tile = ctx->opt.judge_general ? 64u : 1024u;
    ctx->timer.begin("judge:rows", S);
    JudgeStat* dst = nullptr; JudgeStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    rows_launch_by_len(S, ctx->opt.judge_general, in->row_len, n, JR_ITER, k_judge_rows<16>, k_judge_rows<64>, k_judge_rows_long, ji, dst);
    KCHK(ctx, "k_judge_rows");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) return rc;
    res->n_kept = hs.c[0]; res->why_short = hs.c[1]; res->why_n = hs.c[2]; res->why_meanq = hs.c[3]; res->why_lowq = hs.c[4]; res->why_complex = hs.c[5];
    res->bases_in = hs.c[6]; res->qsum_in = hs.c[7]; res->q20_in = hs.c[8]; res->q30_in = hs.c[9];
    res->bases_out = hs.c[10]; res->qsum_out = hs.c[11]; res->q20_out = hs.c[12]; res->q30_out = hs.c[13];
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows -> the length adapter removal leaves, insert sizes, a summary: rfq_adapter_rows of include/rfq_hip.h
// One kernel (rows_launch_by_len; RFQ_ADAPTER=general: the wave-per-pair kernel that compares byte by byte, enc/rows_adapter.h) and one read-back, like rfq_judge_rows.
// The adapters come as host bytes and travel as two class planes of 64 bits in the kernel arguments.
static int adapter_planes(rfq_ctx* ctx, const uint8_t* h, uint32_t m, const char* what, unsigned long long* H, unsigned long long* L, uint32_t* len) {
    *H = *L = 0ull; *len = 0u;
    if (!h || !m) return RFQ_OK;
    if (m > 64u) return rfq_fail(ctx, RFQ_E_ARG, "%s has %u bases: an adapter has at most 64", what, m);
    for (uint32_t j = 0; j < m; j++) {
        unsigned long long c;
        switch (h[j] & 0xDFu) { case 'A': c = 0; break; case 'C': c = 1; break; case 'G': c = 2; break; case 'T': c = 3; break;
        default: return rfq_fail(ctx, RFQ_E_ARG, "%s holds a byte that is not one of ACGTacgt (0x%02x at %u)", what, h[j], j); }
        *H |= (c >> 1) << j; *L |= (c & 1ull) << j;
    }
    *len = m;
    return RFQ_OK;
}
extern "C" int rfq_adapter_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_adapter_rows_args* a, rfq_adapter_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    if (a->pairs && (a->min_overlap == 0u || a->max_diff_pct > 100u)) return rfq_fail(ctx, RFQ_E_ARG, "with pairs min_overlap is >= 1 and max_diff_pct 0 .. 100 (got %u, %u)", a->min_overlap, a->max_diff_pct);
    if (!a->pairs && ((a->h_adapter2 && a->adapter2_len) || a->d_insert || a->d_diff || a->d_insert_hist))
        return rfq_fail(ctx, RFQ_E_ARG, "h_adapter2, d_insert, d_diff and d_insert_hist are for pairs");
    AdapterIn ai; memset(&ai, 0, sizeof ai);
    if ((rc = adapter_planes(ctx, a->h_adapter1, a->adapter1_len, "adapter 1", &ai.a_h[0], &ai.a_l[0], &ai.a_m[0])) != RFQ_OK) return rc;
    if ((rc = adapter_planes(ctx, a->h_adapter2, a->adapter2_len, "adapter 2", &ai.a_h[1], &ai.a_l[1], &ai.a_m[1])) != RFQ_OK) return rc;
    if ((ai.a_m[0] || ai.a_m[1]) && (a->adapter_min < 1u || a->adapter_min > 64u)) return rfq_fail(ctx, RFQ_E_ARG, "adapter_min must be 1 .. 64 with an adapter (got %u)", a->adapter_min);
    if (a->hist_len > 65536u || (a->d_insert_hist && a->hist_len == 0u)) return rfq_fail(ctx, RFQ_E_ARG, "hist_len must be 1 .. 65536 with d_insert_hist, at most 65536 without (got %u)", a->hist_len);
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if (n && (!in->d_lens || !in->d_bases)) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens / d_bases");
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_len | (uintptr_t)a->d_insert | (uintptr_t)a->d_diff) & 3u)
        return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_len, d_insert and d_diff must be 4-byte aligned");
    if ((uintptr_t)a->d_insert_hist & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_insert_hist must be 8-byte aligned");
    const uint64_t units = a->pairs ? n / 2 : n;
    {
        Span ins[5]; rows_src_spans(in, false, ins);
        ins[1].p = nullptr;                                                  // (the scores are not read)
        const Span outs[] = { { a->d_len, n * 4ull, "d_len" }, { a->d_how, n, "d_how" }, { a->d_insert, units * 4ull, "d_insert" }, { a->d_diff, units * 4ull, "d_diff" },
                              { a->d_insert_hist, a->hist_len * 8ull, "d_insert_hist" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
    }
    res->n_rows = n; res->n_pairs = a->pairs ? units : 0;
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    if ((rc = rows_hist_fresh(ctx, S, a->d_insert_hist, a->hist_len, n)) != RFQ_OK || !n) return rc;
    ai.b = in->d_bases; ai.lens = in->d_lens; ai.total = n * in->row_len; ai.n_rows = (uint32_t)n; ai.n_units = (uint32_t)units; ai.row_len = in->row_len;
    ai.vec_in = rows_vec(in->row_len, in->d_bases, nullptr);
    ai.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u; ai.pairs = a->pairs ? 1u : 0u;
    ai.min_overlap = a->min_overlap; ai.max_diff = a->max_diff; ai.max_diff_pct = a->max_diff_pct;
    if (!a->pairs) { ai.a_h[1] = ai.a_l[1] = 0ull; ai.a_m[1] = 0u; }
    ai.adapter_min = a->adapter_min; ai.adapter_mm_per = a->adapter_mm_per; ai.hist_len = a->hist_len;
    ai.len = a->d_len; ai.how = a->d_how; ai.insert = a->d_insert; ai.diff = a->d_diff; ai.hist = (unsigned long long*)a->d_insert_hist;
    ctx->timer.begin("adapter:rows", S);
    AdapterStat* dst = nullptr; AdapterStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    rows_launch_by_len(S, ctx->opt.adapter_general, in->row_len, units, AR_ITER, k_adapter_rows<16>, k_adapter_rows<64>, k_adapter_rows_any, ai, dst);
    KCHK(ctx, "k_adapter_rows");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) return rc;
    res->pairs_found = hs.c[0]; res->rows_cut = hs.c[1]; res->rows_cut_overlap = hs.c[2]; res->rows_cut_adapter = hs.c[3]; res->bases_in = hs.c[4]; res->bases_out = hs.c[5];
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows -> a keep byte that leaves one unit of every class of identical units: rfq_dedup_rows of include/rfq_hip.h
// Three kernels and one read-back (enc/rows_dedup.h): the key kernel (which one: rows_launch_by_len) leaves a fingerprint and a score per
// unit, the claim kernel finds every candidate's class in a hash table of S slots, the resolve kernel writes the outputs.  The table lives in context-owned buffers
// and is sized and zeroed PER CALL: a table carried across the batches of one file is not offered (include/rfq_hip.h).
extern "C" int rfq_dedup_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_dedup_rows_args* a, rfq_dedup_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    if (a->mode != RFQ_DEDUP_FIRST && a->mode != RFQ_DEDUP_BEST_QUAL) return rfq_fail(ctx, RFQ_E_ARG, "unknown mode %d", a->mode);
    const bool best = a->mode == RFQ_DEDUP_BEST_QUAL;
    if (n && best && !in->d_quals) return rfq_fail(ctx, RFQ_E_ARG, "RFQ_DEDUP_BEST_QUAL needs rows->d_quals");
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (in->row_len > (1u << 22)) return rfq_fail(ctx, RFQ_E_ARG, "row_len is at most 2^22 = %u: the score is a 32-bit sum (got %u)", 1u << 22, in->row_len);
    const uint64_t units = a->pairs ? n / 2 : n;
    if (units >= 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many units for one call (%llu)", (unsigned long long)units);
    if (n && (!in->d_lens || !in->d_bases)) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens / d_bases");
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_dup_of | (uintptr_t)a->d_count) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_dup_of and d_count must be 4-byte aligned");
    if ((uintptr_t)a->d_hist & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_hist must be 8-byte aligned");
    if (a->hist_len > DD_HIST_MAX || (a->d_hist && a->hist_len == 0u)) return rfq_fail(ctx, RFQ_E_ARG, "hist_len must be 1 .. %u with d_hist, at most %u without (got %u)", DD_HIST_MAX, DD_HIST_MAX, a->hist_len);
    {
        Span ins[6]; rows_src_spans(in, false, ins);
        if (!best) ins[1].p = nullptr;                                       // (the scores are read in BEST_QUAL only)
        ins[5] = { a->d_in, n, "d_in" };
        const Span outs[] = { { a->d_keep, n, "d_keep" }, { a->d_dup_of, units * 4ull, "d_dup_of" }, { a->d_count, units * 4ull, "d_count" }, { a->d_hist, a->hist_len * 8ull, "d_hist" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
    }
    res->n_units = units;
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    if ((rc = rows_hist_fresh(ctx, S, a->d_hist, a->hist_len, n)) != RFQ_OK || !n) return rc;
    uint64_t slots = 1024;
    while (slots < 2 * units) slots <<= 1;
    DedupIn di; memset(&di, 0, sizeof di);
    {
        struct Want { DBuf* d; unsigned long long bytes; } const want[] = { { &ctx->dedup_fp, units * 8ull }, { &ctx->dedup_score, units * 4ull }, { &ctx->dedup_slot, units * 4ull },
                                                                            { &ctx->dedup_tab, slots * 8ull }, { &ctx->dedup_best, slots * 8ull }, { &ctx->dedup_cnt, slots * 4ull } };
        for (const Want& w : want)
            if (const hipError_t e = w.d->ensure((size_t)w.bytes); e != hipSuccess) {
                (void)hipGetLastError();
                return rfq_fail(ctx, RFQ_E_HIP, "the table of %llu slots for %llu units needs %llu bytes of device memory (a buffer of %llu bytes could not be had): %s",
                                (unsigned long long)slots, (unsigned long long)units, (unsigned long long)(slots * 20ull + units * 16ull), w.bytes, hipGetErrorString(e));
            }
    }
    di.b = in->d_bases; di.q = best ? in->d_quals : nullptr; di.lens = in->d_lens; di.cand = a->d_in; di.total = n * in->row_len;
    di.n_rows = (uint32_t)n; di.n_units = (uint32_t)units; di.row_len = in->row_len; di.vec_in = rows_vec(in->row_len, in->d_bases, di.q);
    di.pairs = a->pairs ? 1u : 0u; di.key_len = a->key_len; di.collide = ctx->opt.dedup_collide ? 1u : 0u; di.hist_len = a->hist_len;
    di.fp = ctx->dedup_fp.as<unsigned long long>(); di.score = ctx->dedup_score.as<uint32_t>(); di.slot = ctx->dedup_slot.as<uint32_t>();
    di.tab = ctx->dedup_tab.as<unsigned long long>(); di.best = ctx->dedup_best.as<unsigned long long>(); di.cnt = ctx->dedup_cnt.as<uint32_t>(); di.S = slots;
    di.keep = a->d_keep; di.dup_of = a->d_dup_of; di.count = a->d_count; di.hist = (unsigned long long*)a->d_hist;
    const uint32_t ublocks = (uint32_t)((units + 255u) / 256u);
    ctx->timer.begin("dedup:key", S);
    { ClearList z; memset(&z, 0, sizeof z); z.add(di.tab, slots * 8, 0u); z.add(di.best, slots * 8, 0u); z.add(di.cnt, slots * 4, 0u); clear_list(S, z); KCHK(ctx, "k_clear_list"); }
    DedupStat* dst = nullptr; DedupStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    rows_launch_by_len(S, false, in->row_len, units, DD_ITER, k_dedup_key<16>, k_dedup_key<64>, k_dedup_key_long, di, dst);
    KCHK(ctx, "k_dedup_key");
    ctx->timer.end(S);
    ctx->timer.begin("dedup:claim", S);
    hipLaunchKernelGGL(k_dedup_claim, dim3(ublocks), dim3(256), 0, S, di);
    KCHK(ctx, "k_dedup_claim");
    ctx->timer.end(S);
    ctx->timer.begin("dedup:resolve", S);
    hipLaunchKernelGGL(k_dedup_resolve, dim3(ublocks), dim3(256), 0, S, di, dst);
    KCHK(ctx, "k_dedup_resolve");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) return rc;
    res->n_candidates = hs.c[0]; res->bases_in = hs.c[1]; res->n_classes = hs.c[2]; res->bases_kept = hs.c[3]; res->max_class = hs.c[4]; res->n_dups = hs.c[0] - hs.c[2];
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows under a keep / start / length triple -> the tables of a QC report: rfq_profile_rows of include/rfq_hip.h
// One kernel and one read-back (enc/rows_profile.h).  Rows of up to 1024 bytes whose tables fit a compute unit's LDS go to k_profile_rows<16> / <64>: the grid is
// PF_WG_PER_CU workgroups per compute unit - a workgroup pays for its table once, at its end - and the steps each takes follow from that; beyond PF_ROWS_MAX rows
// per workgroup (the bound of a 32-bit cell) the grid grows instead.  Everything else (and RFQ_PROFILE=general) goes to the wave-per-row kernel.
static int profile_win_refusal(rfq_ctx* ctx, unsigned long long row) {
    return rfq_fail(ctx, RFQ_E_ARG, "a window is negative or ends behind its read: start < 0, len < 0 or start + len > lens[i] (first such row: %llu)", row);
}
extern "C" int rfq_profile_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_profile_rows_args* a, rfq_profile_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    const bool per_cycle = a->d_base_cnt || a->d_base_qsum || a->d_qual_hist, per_score = a->d_qual_hist || a->d_meanq_hist;
    if (per_cycle && (a->cycles < 1u || a->cycles > 65536u)) return rfq_fail(ctx, RFQ_E_ARG, "cycles must be 1 .. 65536 with a per-cycle table (got %u)", a->cycles);
    if (per_score && (a->qbins < 1u || a->qbins > 256u)) return rfq_fail(ctx, RFQ_E_ARG, "qbins must be 1 .. 256 with d_qual_hist or d_meanq_hist (got %u)", a->qbins);
    if (a->d_len_hist && (a->len_bins < 1u || a->len_bins > (1u << 20))) return rfq_fail(ctx, RFQ_E_ARG, "len_bins must be 1 .. 2^20 with d_len_hist (got %u)", a->len_bins);
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    if (n && !in->d_lens) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens");
    if (n && !in->d_quals && (a->d_base_qsum || a->d_qual_hist || a->d_meanq_hist)) return rfq_fail(ctx, RFQ_E_ARG, "d_base_qsum, d_qual_hist and d_meanq_hist need rows->d_quals");
    if (n && !in->d_bases && (a->d_base_cnt || a->d_base_qsum || a->d_gc_hist)) return rfq_fail(ctx, RFQ_E_ARG, "d_base_cnt, d_base_qsum and d_gc_hist need rows->d_bases");
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_start | (uintptr_t)a->d_len) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_start and d_len must be 4-byte aligned");
    if (((uintptr_t)a->d_base_cnt | (uintptr_t)a->d_base_qsum | (uintptr_t)a->d_qual_hist | (uintptr_t)a->d_len_hist | (uintptr_t)a->d_meanq_hist | (uintptr_t)a->d_gc_hist) & 7u)
        return rfq_fail(ctx, RFQ_E_ARG, "the tables must be 8-byte aligned");
    const unsigned long long M = a->pairs ? 2ull : 1ull;
    const Span outs[] = { { a->d_base_cnt, M * a->cycles * 40ull, "d_base_cnt" }, { a->d_base_qsum, M * a->cycles * 40ull, "d_base_qsum" },
                          { a->d_qual_hist, M * a->cycles * a->qbins * 8ull, "d_qual_hist" }, { a->d_len_hist, M * a->len_bins * 8ull, "d_len_hist" },
                          { a->d_meanq_hist, M * a->qbins * 8ull, "d_meanq_hist" }, { a->d_gc_hist, M * PF_GC_BINS * 8ull, "d_gc_hist" } };
    {
        Span ins[8]; rows_src_spans(in, false, ins);
        ins[5] = { a->d_keep, n, "d_keep" }; ins[6] = { a->d_start, n * 4ull, "d_start" }; ins[7] = { a->d_len, n * 4ull, "d_len" };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK || (rc = rows_outs_apart(ctx, outs)) != RFQ_OK) return rc;
    }
    res->n_rows = n;
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    for (const Span& o : outs) if (o.p) HIPCHK(ctx, hipMemsetAsync(const_cast<void*>(o.p), 0, (size_t)o.n, S));
    if (!n) { HIPCHK(ctx, hipStreamSynchronize(S)); return RFQ_OK; }
    ProfileIn pi; memset(&pi, 0, sizeof pi);
    pi.b = in->d_bases; pi.q = in->d_quals; pi.lens = in->d_lens; pi.keep = a->d_keep; pi.start = a->d_start; pi.len = a->d_len;
    pi.total = n * in->row_len; pi.n_rows = (uint32_t)n; pi.row_len = in->row_len; pi.vec_in = rows_vec(in->row_len, in->d_bases, in->d_quals);
    pi.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u; pi.pairs = a->pairs ? 1u : 0u;
    pi.cycles = per_cycle ? a->cycles : 1u; pi.qbins = per_score ? a->qbins : 1u; pi.len_bins = a->d_len_hist ? a->len_bins : 1u;
    pi.base_cnt = (unsigned long long*)a->d_base_cnt; pi.base_qsum = (unsigned long long*)a->d_base_qsum; pi.qual_hist = (unsigned long long*)a->d_qual_hist;
    pi.len_hist = (unsigned long long*)a->d_len_hist; pi.meanq_hist = (unsigned long long*)a->d_meanq_hist; pi.gc_hist = (unsigned long long*)a->d_gc_hist;
    pi.tile = ctx->opt.profile_general ? 64u : 1024u;
    // the common path's LDS: a table that is not asked for takes no room (enc/rows_profile.h has the layout)
    pi.ch = (pi.cycles + 15u) / 16u; pi.qs = pi.qbins | 1u;
    unsigned long long words = 0;
    const unsigned long long cs = 16ull * pi.ch;
    pi.o_base = 0u; if (a->d_base_cnt || a->d_base_qsum) words += cs * 10ull;
    pi.o_qh = (uint32_t)words; if (a->d_qual_hist) words += cs * pi.qs;
    pi.o_len = (uint32_t)words; if (a->d_len_hist) words += pi.len_bins;
    pi.o_mq = (uint32_t)words; if (a->d_meanq_hist) words += pi.qbins;
    pi.o_gc = (uint32_t)words; if (a->d_gc_hist) words += PF_GC_BINS;
    words += words & 1ull;
    const bool lds = !ctx->opt.profile_general && in->row_len <= 1024u && words * 4ull <= PF_LDS_MAX;
    ctx->timer.begin("profile:rows", S);
    ProfileStat* dst = nullptr; ProfileStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if (lds) {
        const uint32_t R = in->row_len <= 256u ? 16u : 4u;                    // rows a step
        const uint64_t units = n / M;
        const uint64_t steps = rows_steps_for(units, R, PF_WG_PER_CU * ctx->n_cu / (uint32_t)M, 1u, PF_ROWS_MAX / R);       // (the cap: workgroups of a mate)
        pi.steps = (uint32_t)steps; pi.lds_words = (uint32_t)words;
        const auto k = in->row_len <= 256u ? k_profile_rows<16> : k_profile_rows<64>;
        hipLaunchKernelGGL(k, dim3(rows_steps_grid(units, R, steps) * (uint32_t)M), dim3(256), (size_t)words * 4u, S, pi, dst);
    } else hipLaunchKernelGGL(k_profile_rows_long, dim3((uint32_t)n), dim3(64), 0, S, pi, dst);
    KCHK(ctx, "k_profile_rows");
    ctx->timer.end(S);
    rc = rows_sums_back(ctx, S, dst, &hs, in->row_len);                      // (a bad length refuses; a bad window in a row in front of it, or alone, is the one to name)
    if ((hs.err & PF_ERR_WIN) && (rc == RFQ_OK || ~hs.c[15] < hs.bad_row)) return profile_win_refusal(ctx, ~hs.c[15]);
    if (rc != RFQ_OK) return rc;
    for (int m = 0; m < 2; m++) {
        const unsigned long long* c = hs.c + 7 * m;
        res->counted[m] = c[0]; res->bases[m] = c[1]; res->qsum[m] = c[2]; res->q20[m] = c[3]; res->q30[m] = c[4]; res->gc[m] = c[5]; res->other[m] = c[6];
    }
    res->max_len = hs.c[14];
    return RFQ_OK;
}
// ---------------------------------------------------------------- references -> an index of canonical k-mers, rows against it -> k-mers, hits, a keep byte: rfq_screen_build, rfq_screen_rows of include/rfq_hip.h
// The index is the CALLER's (enc/rows_screen.h has its layout): nothing of a screen outlives the call.  The build is two small kernels and one read-back; the rows
// call reads the index's header back, then one kernel (by row length; with the table in LDS where it fits) and one read-back, like rfq_judge_rows.
static uint64_t screen_slots(uint64_t refs_len) { uint64_t s = 1024; while (s < 2 * refs_len) s <<= 1; return s; }
extern "C" int rfq_screen_build(rfq_ctx* ctx, const rfq_screen_build_args* a, rfq_screen_build_result* res) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (a->k < SC_K_MIN || a->k > SC_K_MAX) return rfq_fail(ctx, RFQ_E_ARG, "k must be %u .. %u (got %u)", SC_K_MIN, SC_K_MAX, a->k);
    if (a->n_refs && (!a->d_refs || !a->d_ref_off)) return rfq_fail(ctx, RFQ_E_ARG, "null d_refs / d_ref_off with references");
    if ((uintptr_t)a->d_ref_off & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_ref_off must be 8-byte aligned");
    if ((uintptr_t)a->d_index & 15u) return rfq_fail(ctx, RFQ_E_ARG, "d_index must be 16-byte aligned");
    const uint64_t refs_len = a->n_refs ? a->refs_len : 0;
    if (refs_len >= (1ull << 38) || a->n_refs >= (1ull << 38)) return rfq_fail(ctx, RFQ_E_ARG, "too many reference bytes or references for one index (%llu, %llu)", (unsigned long long)refs_len, (unsigned long long)a->n_refs);
    const uint64_t slots = screen_slots(refs_len), need = sizeof(ScreenHdr) + 8ull * slots;
    res->n_refs = a->n_refs; res->slots = slots; res->index_bytes = need;
    if (a->size_only) return RFQ_OK;
    if (!a->d_index) return rfq_fail(ctx, RFQ_E_ARG, "null d_index");
    if (a->index_cap < need) {
        memset(res, 0, sizeof *res);
        return rfq_fail(ctx, RFQ_E_NOSPACE, "index buffer too small: need %llu bytes (%llu slots)", (unsigned long long)need, (unsigned long long)slots);
    }
    int rc;
    {
        const Span outs[] = { { a->d_index, need, "d_index" } }; const Span ins[] = { { a->d_refs, refs_len, "d_refs" }, { a->d_ref_off, (a->n_refs + 1) * 8ull, "d_ref_off" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
    }
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    ScreenBuildIn bi; memset(&bi, 0, sizeof bi);
    bi.blob = a->d_refs; bi.off = (const unsigned long long*)a->d_ref_off; bi.refs_len = refs_len; bi.n_refs = a->n_refs; bi.k = a->k; bi.collide = ctx->opt.screen == RfqOpts::SCREEN_COLLIDE ? 1u : 0u;
    bi.hdr = (ScreenHdr*)a->d_index; bi.tab = (unsigned long long*)((uint8_t*)a->d_index + sizeof(ScreenHdr)); bi.S = slots;
    ctx->timer.begin("screen:build", S);
    HIPCHK(ctx, hipMemsetAsync(a->d_index, 0, (size_t)need, S));
    ScreenBuildStat* dst = nullptr; ScreenBuildStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if (a->n_refs) { hipLaunchKernelGGL(k_screen_refs, dim3((uint32_t)((a->n_refs + 255u) / 256u)), dim3(256), 0, S, bi, dst); KCHK(ctx, "k_screen_refs"); }
    hipLaunchKernelGGL(k_screen_build, dim3((uint32_t)std::max<uint64_t>(1, (refs_len + 255u) / 256u)), dim3(256), 0, S, bi, dst);
    KCHK(ctx, "k_screen_build");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, 0u)) != RFQ_OK) return rc;
    if (hs.err & SC_ERR_REFS) {
        const unsigned long long br = hs.bad_row;
        memset(res, 0, sizeof *res);
        return rfq_fail(ctx, RFQ_E_ARG, "the reference offsets decrease or end past refs_len = %llu (first such reference: %llu)", (unsigned long long)refs_len, br);
    }
    res->ref_bases = hs.c[0]; res->n_positions = hs.c[1]; res->n_kmers = hs.c[2];
    return RFQ_OK;
}
extern "C" int rfq_screen_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_screen_rows_args* a, rfq_screen_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    if (a->mode != RFQ_SCREEN_DROP_MATCHED && a->mode != RFQ_SCREEN_KEEP_MATCHED) return rfq_fail(ctx, RFQ_E_ARG, "unknown mode %d", a->mode);
    if (a->min_pct > 100u) return rfq_fail(ctx, RFQ_E_ARG, "min_pct must be 0 .. 100 (got %u)", a->min_pct);
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n && (!in->d_lens || !in->d_bases)) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens / d_bases");
    if (!a->d_index || ((uintptr_t)a->d_index & 15u) || a->index_bytes < sizeof(ScreenHdr)) return rfq_fail(ctx, RFQ_E_ARG, "d_index must be an index of rfq_screen_build: not NULL, 16-byte aligned, at least %zu bytes", sizeof(ScreenHdr));
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_kmers | (uintptr_t)a->d_hits) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_kmers and d_hits must be 4-byte aligned");
    const uint64_t units = a->pairs ? n / 2 : n;
    const Span outs[] = { { a->d_kmers, n * 4ull, "d_kmers" }, { a->d_hits, n * 4ull, "d_hits" }, { a->d_keep, n, "d_keep" } };
    {
        Span ins[7]; rows_src_spans(in, false, ins);
        ins[1].p = nullptr;                                                  // (the scores are not read)
        ins[5] = { a->d_in, n, "d_in" }; ins[6] = { a->d_index, a->index_bytes, "d_index" };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
    }
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    ScreenHdr hd; memset(&hd, 0, sizeof hd);
    HIPCHK(ctx, ctx->fetch(&hd, a->d_index, sizeof hd, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    if (hd.magic != SC_MAGIC || hd.version != SC_VERSION) return rfq_fail(ctx, RFQ_E_DATA, "d_index does not begin with the header rfq_screen_build writes");
    if (hd.k < SC_K_MIN || hd.k > SC_K_MAX) return rfq_fail(ctx, RFQ_E_DATA, "the index's k is %u: not in %u .. %u", hd.k, SC_K_MIN, SC_K_MAX);
    if (hd.S == 0 || (hd.S & (hd.S - 1)) || hd.S > (a->index_bytes - sizeof(ScreenHdr)) / 8u)
        return rfq_fail(ctx, RFQ_E_DATA, "the index's slot count %llu is no power of two or exceeds index_bytes = %zu", (unsigned long long)hd.S, a->index_bytes);
    res->n_units = units;
    if (!n) return RFQ_OK;
    ScreenIn si; memset(&si, 0, sizeof si);
    si.b = in->d_bases; si.lens = in->d_lens; si.cand = a->d_in; si.total = n * in->row_len; si.n_rows = (uint32_t)n; si.n_units = (uint32_t)units; si.row_len = in->row_len;
    si.vec_in = rows_vec(in->row_len, in->d_bases, nullptr);
    si.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u; si.pairs = a->pairs ? 1u : 0u; si.keep_matched = a->mode == RFQ_SCREEN_KEEP_MATCHED ? 1u : 0u;
    si.min_hits = a->min_hits; si.min_pct = a->min_pct; si.k = hd.k; si.collide = hd.flags & SC_FLAG_COLLIDE ? 1u : 0u;
    si.tab = (const unsigned long long*)((const uint8_t*)a->d_index + sizeof(ScreenHdr)); si.S = hd.S;
    si.kmers = a->d_kmers; si.hits = a->d_hits; si.keep = a->d_keep;
    const bool general = ctx->opt.screen == RfqOpts::SCREEN_GENERAL, lds = !general && in->row_len <= 1024u && hd.S >= 2u && hd.S <= SC_LDS_SLOTS;
    ctx->timer.begin("screen:rows", S);
    ScreenStat* dst = nullptr; ScreenStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if (lds) {
        // a workgroup pays for its copy of the slots once: at most two workgroups per compute unit (one where the slots take more than 64 KiB), the steps follow
        const uint32_t R = (uint32_t)SC_LDS_NT / (in->row_len <= 256u ? 16u : 64u);
        const uint64_t steps = rows_steps_for(units, R, ctx->n_cu * (hd.S * 8u <= 65536u ? 2u : 1u), 1u, UINT64_MAX);
        si.steps = (uint32_t)steps;
        const auto k = in->row_len <= 256u ? k_screen_rows<16, SC_LDS_NT, true> : k_screen_rows<64, SC_LDS_NT, true>;
        hipLaunchKernelGGL(k, dim3(rows_steps_grid(units, R, steps)), dim3(SC_LDS_NT), (size_t)hd.S * 8u, S, si, dst);
    } else {
        si.steps = SC_ITER;
        rows_launch_by_len(S, general, in->row_len, units, SC_ITER, k_screen_rows<16, 256, false>, k_screen_rows<64, 256, false>, k_screen_rows_long, si, dst);
    }
    KCHK(ctx, "k_screen_rows");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    res->n_candidates = hs.c[0]; res->n_matched = hs.c[1]; res->n_kept = hs.c[2]; res->kmers = hs.c[3]; res->hits = hs.c[4]; res->bases_in = hs.c[5]; res->bases_kept = hs.c[6];
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows -> a table of canonical k-mers with counts that adds up across calls, and its reader: rfq_kmers_init, rfq_kmers_rows, rfq_kmers_read of include/rfq_hip.h
// The table is the CALLER's (enc/rows_kmers.h has its layout) and is the one thing of the rows family that outlives a call.  rfq_kmers_rows reads the header back, runs
// one kernel (by row length and RFQ_KMERS) and a one-thread kernel that carries the call's sums into the header, then one read-back; rfq_kmers_read is a count pass,
// a read-back - room is judged before anything is written - and a writing pass.
static uint64_t kmers_pow2(uint64_t want) { uint64_t s = 1024; while (s < want) s <<= 1; return s; }
extern "C" int rfq_kmers_init(rfq_ctx* ctx, const rfq_kmers_init_args* a, rfq_kmers_init_result* res) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    if (a->k < SC_K_MIN || a->k > SC_K_MAX) return rfq_fail(ctx, RFQ_E_ARG, "k must be %u .. %u (got %u)", SC_K_MIN, SC_K_MAX, a->k);
    if (a->slots > (1ull << 36)) return rfq_fail(ctx, RFQ_E_ARG, "slots is at most 2^36 (got %llu)", (unsigned long long)a->slots);
    const bool collide = ctx->opt.kmers == RfqOpts::KMERS_COLLIDE;
    const uint64_t S = kmers_pow2(a->slots), need = sizeof(KmersHdr) + 16ull * S;
    if (collide && S > KM_COLLIDE_SLOTS) return rfq_fail(ctx, RFQ_E_ARG, "RFQ_KMERS=collide takes at most %u slots: its probe chains are as long as the table is full (got %llu)", KM_COLLIDE_SLOTS, (unsigned long long)S);
    if ((uintptr_t)a->d_table & 15u) return rfq_fail(ctx, RFQ_E_ARG, "d_table must be 16-byte aligned");
    res->slots = S; res->table_bytes = need;
    if (a->size_only) return RFQ_OK;
    if (!a->d_table) { memset(res, 0, sizeof *res); return rfq_fail(ctx, RFQ_E_ARG, "null d_table"); }
    if (a->table_cap < need) {
        memset(res, 0, sizeof *res);
        return rfq_fail(ctx, RFQ_E_NOSPACE, "table buffer too small: need %llu bytes (%llu slots)", (unsigned long long)need, (unsigned long long)S);
    }
    hipStream_t St = ctx->stream; int rc;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    ctx->timer.begin("kmers:init", St);
    HIPCHK(ctx, hipMemsetAsync(a->d_table, 0, (size_t)need, St));
    hipLaunchKernelGGL(k_kmers_format, dim3(1), dim3(64), 0, St, (KmersHdr*)a->d_table, a->k, (unsigned long long)S, collide ? KM_FLAG_COLLIDE : 0u);
    KCHK(ctx, "k_kmers_format");
    ctx->timer.end(St);
    HIPCHK(ctx, hipStreamSynchronize(St));
    ctx->timer.collect();
    return RFQ_OK;
}
// the table's header back on the host and judged: what rfq_kmers_rows and rfq_kmers_read do first (one read-back)
static int kmers_header(rfq_ctx* ctx, hipStream_t S, const void* d_table, size_t table_bytes, KmersHdr* hd) {
    memset(hd, 0, sizeof *hd);
    HIPCHK(ctx, ctx->fetch(hd, d_table, sizeof *hd, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    if (hd->magic != KM_MAGIC || hd->version != KM_VERSION) return rfq_fail(ctx, RFQ_E_DATA, "d_table does not begin with the header rfq_kmers_init writes");
    if (hd->k < SC_K_MIN || hd->k > SC_K_MAX) return rfq_fail(ctx, RFQ_E_DATA, "the table's k is %u: not in %u .. %u", hd->k, SC_K_MIN, SC_K_MAX);
    if (hd->S == 0 || (hd->S & (hd->S - 1)) || hd->S > (table_bytes - sizeof(KmersHdr)) / 16u)
        return rfq_fail(ctx, RFQ_E_DATA, "the table's slot count %llu is no power of two or exceeds table_bytes = %zu", (unsigned long long)hd->S, table_bytes);
    if (hd->flags & KM_FLAG_INCOMPLETE)
        return rfq_fail(ctx, RFQ_E_DATA, "the table is INCOMPLETE: an earlier rfq_kmers_rows lost k-mers in it (%llu values in %llu slots); format a larger one with rfq_kmers_init", (unsigned long long)hd->n_kmers, (unsigned long long)hd->S);
    return RFQ_OK;
}
static int kmers_table_arg(rfq_ctx* ctx, const void* d_table, size_t table_bytes) {
    if (!d_table || ((uintptr_t)d_table & 15u) || table_bytes < sizeof(KmersHdr)) return rfq_fail(ctx, RFQ_E_ARG, "d_table must be a table of rfq_kmers_init: not NULL, 16-byte aligned, at least %zu bytes", sizeof(KmersHdr));
    return RFQ_OK;
}
extern "C" int rfq_kmers_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_kmers_rows_args* a, rfq_kmers_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n && (!in->d_lens || !in->d_bases)) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens / d_bases");
    if ((rc = kmers_table_arg(ctx, a->d_table, a->table_bytes)) != RFQ_OK) return rc;
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_kmers) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens and d_kmers must be 4-byte aligned");
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    {
        Span ins[7]; rows_src_spans(in, false, ins);
        ins[1].p = nullptr;                                                  // (the scores are not read)
        ins[5] = { a->d_in, n, "d_in" }; ins[6] = { a->d_table, a->table_bytes, "d_table" };
        const Span outs[] = { { a->d_kmers, n * 4ull, "d_kmers" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK) return rc;
        ins[6].p = nullptr;                                                  // (the table is written too: it lies on none of the call's inputs)
        const Span tab[] = { { a->d_table, a->table_bytes, "d_table" } };
        if ((rc = rows_apart(ctx, tab, ins, "")) != RFQ_OK) return rc;
    }
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    KmersHdr hd;
    if ((rc = kmers_header(ctx, S, a->d_table, a->table_bytes, &hd)) != RFQ_OK) return rc;
    res->n_rows = n; res->n_kmers = hd.n_kmers; res->total = hd.total;
    if (!n) return RFQ_OK;
    KmersIn ki; memset(&ki, 0, sizeof ki);
    ki.b = in->d_bases; ki.lens = in->d_lens; ki.cand = a->d_in; ki.total = n * in->row_len; ki.n_rows = (uint32_t)n; ki.row_len = in->row_len;
    ki.vec_in = rows_vec(in->row_len, in->d_bases, nullptr); ki.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u;
    ki.k = hd.k; ki.collide = hd.flags & KM_FLAG_COLLIDE ? 1u : 0u; ki.walk = (uint32_t)(ki.collide ? std::min<uint64_t>(hd.S, 0xFFFFFFFFull) : std::min<uint64_t>(hd.S, KM_WALK));
    ki.tab = (unsigned long long*)((uint8_t*)a->d_table + sizeof(KmersHdr)); ki.cnt = ki.tab + hd.S; ki.S = hd.S; ki.kmers = a->d_kmers;
    const bool general = ctx->opt.kmers == RfqOpts::KMERS_GENERAL, direct = ctx->opt.kmers == RfqOpts::KMERS_DIRECT;
    // a workgroup pays for the flush of its LDS table once: KM_WG_PER_CU workgroups per compute unit, the steps follow (at least KM_ITER, the family's walk; RFQ_KMERS=direct keeps the same grid)
    ki.steps = (uint32_t)rows_steps_for(n, in->row_len <= 256u ? 16u : 4u, (uint64_t)KM_WG_PER_CU * ctx->n_cu, KM_ITER, KM_STEPS_MAX);
    ctx->timer.begin("kmers:rows", S);
    KmersStat* dst = nullptr; KmersStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if (direct) rows_launch_by_len(S, general, in->row_len, n, ki.steps, k_kmers_rows<16, false>, k_kmers_rows<64, false>, k_kmers_rows_long, ki, dst);
    else rows_launch_by_len(S, general, in->row_len, n, ki.steps, k_kmers_rows<16, true>, k_kmers_rows<64, true>, k_kmers_rows_long, ki, dst);
    KCHK(ctx, "k_kmers_rows");
    hipLaunchKernelGGL(k_kmers_hdr, dim3(1), dim3(64), 0, S, (KmersHdr*)a->d_table, (const KmersStat*)dst);
    KCHK(ctx, "k_kmers_hdr");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    res->n_counted = hs.c[0]; res->bases_in = hs.c[1]; res->added = hs.c[2]; res->n_new = hs.c[3]; res->lost = hs.c[4];
    res->n_kmers = hd.n_kmers + hs.c[3]; res->total = hd.total + hs.c[2];
    if (hs.c[4]) return rfq_fail(ctx, RFQ_E_NOSPACE, "the table is too full: %llu k-mers lost with %llu values in %llu slots; the table is now INCOMPLETE - format one of at least twice the distinct values expected",
                                 (unsigned long long)hs.c[4], (unsigned long long)res->n_kmers, (unsigned long long)hd.S);
    return RFQ_OK;
}
extern "C" int rfq_kmers_read(rfq_ctx* ctx, const rfq_kmers_read_args* a, rfq_kmers_read_result* res) {
    if (!ctx || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    int rc;
    if ((rc = kmers_table_arg(ctx, a->d_table, a->table_bytes)) != RFQ_OK) return rc;
    if (a->hist_len > 65536u || (a->d_hist && a->hist_len == 0u)) return rfq_fail(ctx, RFQ_E_ARG, "hist_len must be 1 .. 65536 with d_hist, at most 65536 without (got %u)", a->hist_len);
    if (((uintptr_t)a->d_hist | (uintptr_t)a->d_values | (uintptr_t)a->d_counts) & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_hist, d_values and d_counts must be 8-byte aligned");
    if ((uintptr_t)a->d_index & 15u) return rfq_fail(ctx, RFQ_E_ARG, "d_index must be 16-byte aligned");
    const bool write = !a->size_only, list = write && (a->d_values || a->d_counts);
    if (write) {
        // (what the call can write at most: the caps are judged against the table's contents below)
        const Span outs[] = { { a->d_hist, a->hist_len * 8ull, "d_hist" }, { a->d_values, (unsigned long long)a->list_cap * 8ull, "d_values" }, { a->d_counts, (unsigned long long)a->list_cap * 8ull, "d_counts" },
                              { a->d_index, a->index_cap, "d_index" } };
        const Span ins[] = { { a->d_table, a->table_bytes, "d_table" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK || (rc = rows_outs_apart(ctx, outs)) != RFQ_OK) return rc;
    }
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    KmersHdr hd;
    if ((rc = kmers_header(ctx, S, a->d_table, a->table_bytes, &hd)) != RFQ_OK) return rc;
    KmersReadIn ri; memset(&ri, 0, sizeof ri);
    ri.tab = (const unsigned long long*)((const uint8_t*)a->d_table + sizeof(KmersHdr)); ri.cnt = ri.tab + hd.S; ri.S = hd.S;
    ri.min_count = std::max<unsigned long long>(a->min_count, 1ull); ri.max_count = a->max_count; ri.k = hd.k;
    const uint32_t blocks = (uint32_t)((hd.S + 256ull * KM_READ_ITER - 1u) / (256ull * KM_READ_ITER));
    ctx->timer.begin("kmers:read", S);
    KmersReadStat* dst = nullptr; KmersReadStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    hipLaunchKernelGGL(k_kmers_count, dim3(blocks), dim3(256), 0, S, ri, dst);
    KCHK(ctx, "k_kmers_count");
    memset(&hs, 0, sizeof hs);
    HIPCHK(ctx, ctx->fetch(&hs, dst, sizeof hs, S));
    HIPCHK(ctx, ctx->fetch_sync(S));
    if (hs.c[0] != hd.n_kmers || hs.c[1] != hd.total) {
        ctx->timer.end(S); HIPCHK(ctx, hipStreamSynchronize(S)); ctx->timer.collect();
        return rfq_fail(ctx, RFQ_E_DATA, "the table's header counts %llu values and %llu occurrences, its slots hold %llu and %llu: it was written over",
                        (unsigned long long)hd.n_kmers, (unsigned long long)hd.total, (unsigned long long)hs.c[0], (unsigned long long)hs.c[1]);
    }
    const uint64_t iS = kmers_pow2(2 * hs.c[2]), ibytes = sizeof(ScreenHdr) + 8ull * iS;
    res->k = hd.k; res->slots = hd.S; res->n_kmers = hs.c[0]; res->total = hs.c[1]; res->n_selected = hs.c[2]; res->selected_total = hs.c[3]; res->max_count = hs.c[4];
    res->index_slots = iS; res->index_bytes = ibytes;
    const bool short_list = list && a->list_cap < hs.c[2], short_index = write && a->d_index && a->index_cap < ibytes;
    if (!write || short_list || short_index || !(a->d_hist || list || a->d_index)) {
        ctx->timer.end(S); HIPCHK(ctx, hipStreamSynchronize(S)); ctx->timer.collect();
        if (write && (short_list || short_index))
            return rfq_fail(ctx, RFQ_E_NOSPACE, "output buffers too small: need %llu list entries, %llu index bytes (%llu slots)", (unsigned long long)hs.c[2], (unsigned long long)ibytes, (unsigned long long)iS);
        return RFQ_OK;
    }
    ri.hist = (unsigned long long*)a->d_hist; ri.hist_len = a->hist_len; ri.values = (unsigned long long*)a->d_values; ri.counts = (unsigned long long*)a->d_counts; ri.list_cap = a->list_cap;
    if (a->d_index) {
        ri.ihdr = (ScreenHdr*)a->d_index; ri.itab = (unsigned long long*)((uint8_t*)a->d_index + sizeof(ScreenHdr)); ri.iS = iS; ri.icollide = ctx->opt.screen == RfqOpts::SCREEN_COLLIDE ? 1u : 0u;
        HIPCHK(ctx, hipMemsetAsync(a->d_index, 0, (size_t)ibytes, S));
    }
    if (a->d_hist) HIPCHK(ctx, hipMemsetAsync(a->d_hist, 0, (size_t)a->hist_len * 8u, S));
    hipLaunchKernelGGL(k_kmers_write, dim3(blocks), dim3(256), 0, S, ri, dst);
    KCHK(ctx, "k_kmers_write");
    ctx->timer.end(S);
    HIPCHK(ctx, hipStreamSynchronize(S));
    ctx->timer.collect();
    return RFQ_OK;
}
// ---------------------------------------------------------------- rows against barcode sets -> a sample per unit, the keep byte and start of rfq_select_rows, counts per sample: rfq_demux_rows of include/rfq_hip.h
// One kernel and one read-back (enc/rows_demux.h).  The sets come as host bytes: they are judged and packed here - 2 bits a base, base j in bits 2j and 2j + 1, W
// words a barcode (1 up to 16 bases, 2 beyond; both sets at the W of the longer) -, the sample sheet becomes a dense [n1][n2] table, and everything goes to the
// device in ONE stream-ordered copy into scratch of the context's that only grows.  RFQ_DEMUX=general launches the byte-by-byte kernel on the same scratch.
static int demux_set_arg(rfq_ctx* ctx, int which, const uint8_t* h, uint32_t n, uint32_t len, uint32_t off, uint32_t skip) {
    if (!h) return rfq_fail(ctx, RFQ_E_ARG, "set %d: null h_bc%d with n%d = %u", which, which, which, n);
    if (n < 1u || n > DM_N_MAX) return rfq_fail(ctx, RFQ_E_ARG, "set %d: the number of barcodes must be 1 .. %u (got %u)", which, DM_N_MAX, n);
    if (len < 1u || len > DM_LEN_MAX) return rfq_fail(ctx, RFQ_E_ARG, "set %d: the barcode length must be 1 .. %u (got %u)", which, DM_LEN_MAX, len);
    if ((unsigned long long)off + len + skip > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "set %d: off + len + skip = %llu does not fit an int32", which, (unsigned long long)off + len + skip);
    return RFQ_OK;
}
// barcode k of the set into W words at dst; a byte that is no base refuses the call
static int demux_pack(rfq_ctx* ctx, int which, const uint8_t* h, uint32_t k, uint32_t len, uint32_t W, uint32_t* dst) {
    for (uint32_t w = 0; w < W; w++) dst[w] = 0u;
    for (uint32_t j = 0; j < len; j++) {
        uint32_t c;
        switch (h[(size_t)k * len + j] & 0xDFu) { case 'A': c = 0; break; case 'C': c = 1; break; case 'G': c = 2; break; case 'T': c = 3; break;
        default: return rfq_fail(ctx, RFQ_E_ARG, "set %d: barcode %u holds a byte that is not one of ACGTacgt (0x%02x at %u)", which, k, h[(size_t)k * len + j], j); }
        dst[j >> 4] |= c << (2u * (j & 15u));
    }
    return RFQ_OK;
}
extern "C" int rfq_demux_rows(rfq_ctx* ctx, const rfq_rows_in* in, const rfq_demux_rows_args* a, rfq_demux_rows_result* res) {
    if (!ctx || !in || !a || !res) return RFQ_E_ARG;
    memset(res, 0, sizeof *res);
    ctx->err.clear();
    const uint64_t n = in->n_rows;
    int rc;
    if ((rc = rows_pairs_arg(ctx, a->pairs, n)) != RFQ_OK) return rc;
    const bool set2 = a->h_bc2 || a->n2;
    if (!a->pairs && (set2 || a->len2 || a->h_pairs || a->skip2 || a->off2)) return rfq_fail(ctx, RFQ_E_ARG, "set 2 (h_bc2, n2, len2, off2, skip2) and h_pairs are for pairs");
    if (a->h_pairs && !set2) return rfq_fail(ctx, RFQ_E_ARG, "h_pairs needs set 2");
    if (!a->h_bc1 && !a->n1) return rfq_fail(ctx, RFQ_E_ARG, "no set 1: h_bc1 and n1 must be given");
    if ((rc = demux_set_arg(ctx, 1, a->h_bc1, a->n1, a->len1, a->off1, a->skip1)) != RFQ_OK) return rc;
    if (set2 && (rc = demux_set_arg(ctx, 2, a->h_bc2, a->n2, a->len2, a->off2, a->skip2)) != RFQ_OK) return rc;
    if (set2 && (unsigned long long)a->n1 * a->n2 > (1ull << 20)) return rfq_fail(ctx, RFQ_E_ARG, "n1 * n2 is at most 2^20 (got %u * %u)", a->n1, a->n2);
    if (a->max_mm > 32u || a->min_delta > 33u) return rfq_fail(ctx, RFQ_E_ARG, "max_mm is at most 32 and min_delta at most 33 (got %u, %u)", a->max_mm, a->min_delta);
    if (a->h_pairs && (a->n_samples < 1u || a->n_samples > 65536u)) return rfq_fail(ctx, RFQ_E_ARG, "n_samples must be 1 .. 65536 with h_pairs (got %u)", a->n_samples);
    const uint32_t nb[2] = { a->n1, set2 ? a->n2 : 0u }, len[2] = { a->len1, set2 ? a->len2 : 0u };
    const uint8_t* const hb[2] = { a->h_bc1, a->h_bc2 };
    const uint32_t W = std::max(len[0], len[1]) <= 16u ? 1u : 2u;
    const uint32_t n_samples = !set2 ? a->n1 : (a->h_pairs ? a->n_samples : a->n1 * a->n2);
    // the blob: packed set 1, packed set 2, the table, the sets' ASCII bytes (8-byte aligned up to the bytes: a two-word barcode is read as one 64-bit word)
    const size_t o_p[2] = { 0, (size_t)nb[0] * W * 4u }, o_tab = o_p[1] + (size_t)nb[1] * W * 4u, tab_bytes = a->h_pairs ? (size_t)nb[0] * nb[1] * 4u : 0u;
    const size_t o_t[2] = { o_tab + tab_bytes, o_tab + tab_bytes + (size_t)nb[0] * len[0] }, blob_bytes = o_t[1] + (size_t)nb[1] * len[1];
    std::vector<uint8_t>& blob = ctx->demux_host;
    blob.assign(blob_bytes + 8u, 0);
    for (int s = 0; s < 2; s++) {
        if (!nb[s]) continue;
        uint32_t* const pk = (uint32_t*)(blob.data() + o_p[s]);
        for (uint32_t k = 0; k < nb[s]; k++) if ((rc = demux_pack(ctx, s + 1, hb[s], k, len[s], W, pk + (size_t)k * W)) != RFQ_OK) return rc;
        // two equal barcodes: equal packed words (the sort is of indices, so that the message names the pair)
        std::vector<uint32_t> order(nb[s]);
        for (uint32_t k = 0; k < nb[s]; k++) order[k] = k;
        const auto key = [&](uint32_t k) { return (unsigned long long)pk[(size_t)k * W] | (W == 2u ? (unsigned long long)pk[(size_t)k * W + 1u] << 32 : 0ull); };
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key(x) != key(y) ? key(x) < key(y) : x < y; });
        for (uint32_t k = 1; k < nb[s]; k++)
            if (key(order[k]) == key(order[k - 1])) return rfq_fail(ctx, RFQ_E_ARG, "set %d: barcodes %u and %u are equal", s + 1, order[k - 1], order[k]);
        memcpy(blob.data() + o_t[s], hb[s], (size_t)nb[s] * len[s]);
    }
    if (a->h_pairs) {
        int32_t* const tab = (int32_t*)(blob.data() + o_tab);
        for (size_t i = 0; i < (size_t)nb[0] * nb[1]; i++) tab[i] = -1;
        for (uint32_t s = 0; s < n_samples; s++) {
            const int32_t i = a->h_pairs[2u * s], j = a->h_pairs[2u * s + 1u];
            if (i < 0 || (uint32_t)i >= nb[0] || j < 0 || (uint32_t)j >= nb[1]) return rfq_fail(ctx, RFQ_E_ARG, "the sample sheet's pair %u is (%d, %d): not in [0, %u) x [0, %u)", s, i, j, nb[0], nb[1]);
            int32_t& cell = tab[(size_t)i * nb[1] + (uint32_t)j];
            if (cell >= 0) return rfq_fail(ctx, RFQ_E_ARG, "the sample sheet lists the pair (%d, %d) twice (samples %d and %u)", i, j, cell, s);
            cell = (int32_t)s;
        }
    }
    if ((rc = rows_base_mode_arg(ctx, in)) != RFQ_OK) return rc;
    if ((rc = rows_src_len_arg(ctx, in, n != 0)) != RFQ_OK) return rc;
    if (n && (!in->d_lens || !in->d_bases)) return rfq_fail(ctx, RFQ_E_ARG, "null d_lens / d_bases");
    if (((uintptr_t)in->d_lens | (uintptr_t)a->d_sample | (uintptr_t)a->d_best | (uintptr_t)a->d_start) & 3u) return rfq_fail(ctx, RFQ_E_ARG, "d_lens, d_sample, d_best and d_start must be 4-byte aligned");
    if ((uintptr_t)a->d_counts & 7u) return rfq_fail(ctx, RFQ_E_ARG, "d_counts must be 8-byte aligned");
    if (n > 0x7FFFFFFFull) return rfq_fail(ctx, RFQ_E_ARG, "too many rows for one call (%llu)", (unsigned long long)n);
    const uint64_t units = a->pairs ? n / 2 : n;
    {
        Span ins[6]; rows_src_spans(in, false, ins);
        ins[1].p = nullptr;                                                  // (the scores are not read)
        ins[5] = { a->d_in, n, "d_in" };
        const Span outs[] = { { a->d_sample, units * 4ull, "d_sample" }, { a->d_why, units, "d_why" }, { a->d_best, n * 4ull, "d_best" }, { a->d_dist, n, "d_dist" }, { a->d_keep, n, "d_keep" },
                              { a->d_start, n * 4ull, "d_start" }, { a->d_counts, ((unsigned long long)n_samples + 1ull) * 8ull, "d_counts" } };
        if ((rc = rows_apart(ctx, outs, ins, "")) != RFQ_OK || (rc = rows_outs_apart(ctx, outs)) != RFQ_OK) return rc;
    }
    res->n_units = units; res->n_samples = n_samples;
    hipStream_t S = ctx->stream;
    if ((rc = rows_begin(ctx)) != RFQ_OK) return rc;
    if ((rc = rows_hist_fresh(ctx, S, a->d_counts, n_samples + 1u, n)) != RFQ_OK || !n) return rc;
    HIPCHK(ctx, ctx->demux_sets.ensure(blob.size()));
    uint8_t* const dblob = ctx->demux_sets.as<uint8_t>();
    DemuxIn di; memset(&di, 0, sizeof di);
    di.b = in->d_bases; di.lens = in->d_lens; di.cand = a->d_in; di.total = n * in->row_len; di.n_rows = (uint32_t)n; di.n_units = (uint32_t)units; di.row_len = in->row_len;
    di.vec_in = rows_vec(in->row_len, in->d_bases, nullptr);
    di.ascii = in->base_mode == RFQ_ROWS_ASCII ? 1u : 0u; di.pairs = a->pairs ? 1u : 0u;
    di.n[0] = nb[0]; di.n[1] = nb[1]; di.len[0] = len[0]; di.len[1] = len[1]; di.off[0] = a->off1; di.off[1] = set2 ? a->off2 : 0u; di.skip[0] = a->skip1; di.skip[1] = set2 ? a->skip2 : 0u;
    di.max_mm = a->max_mm; di.min_delta = a->min_delta; di.n_samples = n_samples;
    for (int s = 0; s < 2; s++) { di.packed[s] = (const uint32_t*)(dblob + o_p[s]); di.text[s] = dblob + o_t[s]; }
    di.table = a->h_pairs ? (const int32_t*)(dblob + o_tab) : nullptr;
    di.sample = a->d_sample; di.why = a->d_why; di.best = a->d_best; di.dist = a->d_dist; di.keep = a->d_keep; di.start = a->d_start; di.counts = (unsigned long long*)a->d_counts;
    ctx->timer.begin("demux:rows", S);
    HIPCHK(ctx, hipMemcpyAsync(dblob, blob.data(), blob.size(), hipMemcpyHostToDevice, S));
    DemuxStat* dst = nullptr; DemuxStat hs;
    if ((rc = rows_stat_fresh(ctx, S, &dst)) != RFQ_OK) return rc;
    if (ctx->opt.demux_general) hipLaunchKernelGGL(k_demux_rows_general, dim3((uint32_t)((units + 255u) / 256u)), dim3(256), 0, S, di, dst);
    else {
        // a workgroup pays for its copy of the sets and the flush of its counts once: DM_WG_PER_CU workgroups per compute unit, the steps follow
        di.lds_counts = a->d_counts && n_samples + 1u <= DM_LDS_COUNTS ? 1u : 0u;
        const uint64_t steps = rows_steps_for(units, 256u, (uint64_t)DM_WG_PER_CU * ctx->n_cu, 1u, UINT64_MAX);
        di.steps = (uint32_t)steps;
        const auto k = W == 1u ? k_demux_rows<1> : k_demux_rows<2>;
        hipLaunchKernelGGL(k, dim3(rows_steps_grid(units, 256u, steps)), dim3(256), ((size_t)(nb[0] + nb[1]) * W + (di.lds_counts ? n_samples + 1u : 0u)) * 4u + 8u, S, di, dst);
    }
    KCHK(ctx, "k_demux_rows");
    ctx->timer.end(S);
    if ((rc = rows_sums_back(ctx, S, dst, &hs, in->row_len)) != RFQ_OK) { memset(res, 0, sizeof *res); return rc; }
    res->n_candidates = hs.c[0]; res->n_assigned = hs.c[1]; res->n_exact = hs.c[2]; res->why_none = hs.c[3]; res->why_ambig = hs.c[4]; res->why_short = hs.c[5]; res->why_combo = hs.c[6];
    res->bases_in = hs.c[7]; res->bases_out = hs.c[8];
    return RFQ_OK;
}
