/*
 * rfq_hip.h — C-ABI of librfq_hip.so, the MI355X (gfx950) engine for repaq's RfqCodec path.
 *
 * The reference (OpenGene/repaq v0.5.1) has no FFI: its seam is the C++ class RfqCodec
 * (src/rfqcodec.h:17-43) driven by Repaq::compress / compressPE / decompress / decompressPE (src/repaq.cpp:262-762).  A GPU engine cannot take
 * vector<Read*>, so each entry point below replaces one RfqCodec/Repaq call at BATCH granularity over raw bytes:
 * FASTQ text in HBM -> .rfq chunk images in HBM and back, bit-identical to what the reference writes.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; every d_* pointer is DEVICE memory (hipMalloc or a torch CUDA
 *     tensor's data_ptr()); h_* pointers are host memory.  Input pointers (FASTQ text, .rfq image) may have any alignment and
 *     any length: a stream of 4 GiB or more is worked through in slices inside the call, the result is the one image / the
 *     one text.  A FASTQ pointer that is not 16-byte aligned is rounded down inside the call: the (up to 15) bytes in front of it are READ
 *     (never interpreted), so they must belong to the same allocation - true of any pointer into a hipMalloc'ed buffer or a torch tensor.
 *     Caller-provided OUTPUT buffers must be 16-byte aligned.
 *   - return 0 (RFQ_OK) or a negative RFQ_E_* code; rfq_last_error(ctx) then holds the reference's error_exit text
 *     (src/util.h:246-249) where the reference has one for the condition.
 *   - one rfq_ctx per (host thread, GPU); distinct contexts may be used concurrently.  A context owns its workspace
 *     and its result buffers; result pointers stay valid until the next call on the same context.
 *   - there is NO CPU fallback: without a usable GPU rfq_create fails with RFQ_E_NO_DEVICE.
 */
#ifndef RFQ_HIP_H
#define RFQ_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RFQ_OK              0
#define RFQ_E_NO_DEVICE    -1   /* no GPU / hip runtime error at create */
#define RFQ_E_HIP          -2   /* a hip call failed (message has the hip error string) */
#define RFQ_E_ARG          -3   /* bad argument */
#define RFQ_E_TEXT         -4   /* (no longer returned: '\r' line ends and blank lines take the normalising path, src/fastqreader.cpp:94-196) */
#define RFQ_E_DATA         -5   /* the reference would error_exit on this input (message = its text) */
#define RFQ_E_FORMAT       -6   /* not a valid .rfq / different ALGORITHM_VER (src/rfqheader.cpp:23-25,40-42) */
#define RFQ_E_UNPINNED     -7   /* input is in a reference-UB zone: refused rather than guessed */
#define RFQ_E_NOSPACE      -8   /* caller-provided output buffer too small (required size is reported) */
#define RFQ_E_STATE        -9   /* call order (e.g. encode continuation without a header) */

/* how the FASTQ streams pair up — Repaq::run, src/repaq.cpp:12-20 */
#define RFQ_SE             0    /* -i           : compress()    */
#define RFQ_PE_TWO_FILES   1    /* -i/-I        : compressPE()  */
#define RFQ_PE_INTERLEAVED 2    /* --interleaved_in             */

#define RFQ_HEADER_MAX     (17 + 255)

typedef struct rfq_ctx rfq_ctx;

/* the library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table */
#define RFQ_API __attribute__((visibility("default")))

/* RfqCodec::RfqCodec / ~RfqCodec (src/rfqcodec.cpp:9-14).  device_id: HIP ordinal. */
RFQ_API int         rfq_create(rfq_ctx** out, int device_id);
RFQ_API void        rfq_destroy(rfq_ctx* ctx);
RFQ_API const char* rfq_last_error(const rfq_ctx* ctx);
/* all work of this context is enqueued on `hip_stream` (a hipStream_t; NULL = the context's own stream) */
RFQ_API int         rfq_set_stream(rfq_ctx* ctx, void* hip_stream);

/* RfqCodec::setHeader (src/rfqcodec.cpp:16-18) from the on-disk header bytes (RfqHeader::read, src/rfqheader.cpp:19-43).
 * mSupportInterleaved is not stored on disk; it is re-derived from BIT_ENCODE_PE_BY_OVERLAP, which makeHeader sets
 * exactly when it is true (src/rfqcodec.cpp:117-122). */
RFQ_API int rfq_set_header(rfq_ctx* ctx, const uint8_t* h_header, size_t header_len);
/* the header currently set / made: RfqHeader::write (src/rfqheader.cpp:84-97) */
RFQ_API int rfq_get_header(rfq_ctx* ctx, uint8_t* h_out /* >= RFQ_HEADER_MAX */, size_t* header_len);
RFQ_API void rfq_clear_header(rfq_ctx* ctx);

typedef struct {
    const uint8_t* d_fq1; size_t n1;      /* stream 1 (R1, or the only / interleaved stream)                          */
    const uint8_t* d_fq2; size_t n2;      /* stream 2 (R2) for RFQ_PE_TWO_FILES, else NULL/0                          */
    int32_t  paired;                      /* RFQ_SE / RFQ_PE_TWO_FILES / RFQ_PE_INTERLEAVED                            */
    uint32_t chunk_bases;                 /* Options::chunkSize = max(100,-k)*1000 (src/main.cpp:69); any value >= 1   */
    int32_t  final;                       /* 1: this is the end of the input: also emit the tail chunk
                                             (src/repaq.cpp:590-624).  0: stop after the last full chunk and report how
                                             many bytes were consumed so the caller can carry the rest into the next
                                             batch.                                                                   */
    int32_t  emit_header;                 /* 1: prefix the result with the file header (first batch of a file)        */
    /* line-break bits (src/repaq.cpp:571-572,683-692): a chunk whose last record ends at absolute
     * file offset >= nolb_from{1,2} gets BIT_HAS_NO_LINE_BREAK_AT_END{,_R2}.  The caller (the Repaq::compress counterpart)
     * passes file_off = offset of this batch in the file and nolb_from = start of the final 1 MiB reader block when the
     * file lacks a trailing '\n', or UINT64_MAX.  */
    uint64_t file_off1, file_off2;
    uint64_t nolb_from1, nolb_from2;
    uint8_t* d_out; size_t out_cap;       /* optional caller buffer for the .rfq bytes; NULL = context-owned result    */
    int32_t  flush_all;                   /* 1: the batch ends exactly on a chunk boundary found by rfq_scan_batch: encode
                                             every record of it (like final) without treating its end as the end of the
                                             input (an unterminated last line is not a line; the 1 MiB reader-block rule
                                             still sees the file continue).  For workers of a multi-GPU host queue.     */
    uint32_t carry_bases;                 /* plan pass of a share of a larger input (rfq_scan_batch): bases the chunk that is open at the start of
                                             this text has already taken from the text in front of it (< chunk_bases); the first chunk
                                             closes at chunk_bases - carry_bases.  0 for an encode (a range starts on a chunk boundary).   */
} rfq_encode_args;

typedef struct {
    const uint8_t* d_rfq;                 /* device pointer to [header?][chunk][chunk]...                              */
    size_t   rfq_len;
    uint32_t n_chunks;
    uint64_t n_reads;                     /* reads encoded (PE: both mates counted, like RfqChunk::mReads)            */
    uint64_t n_bases;
    size_t   consumed1, consumed2;        /* bytes of each stream covered by the emitted chunks                        */
    const uint64_t* h_chunk_off;          /* host array [n_chunks+1]: byte offset of each chunk image in d_rfq         */
    int32_t  input_ended;                 /* 1: the reader met an empty line inside a record: FastqReader::read returns NULL
                                             there (src/fastqreader.cpp:180-191), so the result already holds the tail chunk
                                             and the caller must not feed the rest of the input                          */
    int32_t  reserved;
} rfq_encode_result;

/* RfqCodec::makeHeader (first call without a header; src/rfqcodec.cpp:20-145) + RfqCodec::encodeChunk + RfqChunk::write
 * for every chunk of the batch (src/rfqcodec.cpp:147-586, src/rfqchunk.cpp:230-311), with the chunk cut rule of
 * Repaq::compress (src/repaq.cpp:546-553): cut after the read that brings the running base count to >= chunk_bases. */
RFQ_API int rfq_encode_batch(rfq_ctx* ctx, const rfq_encode_args* args, rfq_encode_result* res);

/* The plan pass of a chunk-parallel encode: line index, read lengths and the cut rule of Repaq::compress
 * (src/repaq.cpp:546-553) only — no header, no coding.  h_end1/2[c] = offset in the caller's stream(s) just past the last
 * record of chunk c (for RFQ_PE_TWO_FILES one array per file, else h_end2 is NULL); a host work queue hands the byte ranges
 * [h_end[c0-1], h_end[c1-1]) to other contexts / GPUs, which encode them with flush_all = 1 and the header of the first
 * range (rfq_get_header -> rfq_set_header); the concatenated images equal the one-shot image.  Takes the same arguments as
 * rfq_encode_batch (final = 0: only full chunks are planned, consumed* says where the next scan starts). */
typedef struct {
    uint32_t n_chunks;
    uint64_t n_reads;
    size_t   consumed1, consumed2;
    const uint64_t* h_end1;               /* host arrays [n_chunks], valid until the next call on the context           */
    const uint64_t* h_end2;
    int32_t  input_ended;                 /* as in rfq_encode_result                                                   */
    uint32_t unit_bases;                  /* bases of every cut unit (a read, or a pair) when they are all the same, else 0: with equal units the
                                             chunk cuts of a share follow from the number of units in front of it (repaq_amd/dist.py)      */
} rfq_scan_result;
RFQ_API int rfq_scan_batch(rfq_ctx* ctx, const rfq_encode_args* args, rfq_scan_result* res);

typedef struct {
    const uint8_t* d_rfq; size_t n;       /* .rfq bytes in HBM                                                          */
    int32_t  has_header;                  /* 1: the image starts with the file header (it is parsed and set)           */
    int32_t  split_pe;                    /* 1: decompressPE (even reads -> out1, odd -> out2; src/repaq.cpp:367-373);
                                             0: decompress (everything to out1 in chunk order; Q14)                    */
    int32_t  final;                       /* 1: the image ends the file: apply the NO_LINE_BREAK bits of the last chunk
                                             (src/repaq.cpp:301-328,375-413)                                           */
    int32_t  bug_compat;                  /* 1: Repaq::decompressPE as it stands (src/repaq.cpp:330-417): with split_pe = 1, a chunk that carries a
                                             NO_LINE_BREAK bit and is not the image's last makes the reference's loop lose the chunk behind it (and, with
                                             the R1 bit, the flagged chunk's R2 text).  0 (default): every read is kept.  With final = 0 a flagged chunk
                                             at the very end of the range stays unconsumed (what follows it decides).  Repaq::decompress (split_pe = 0,
                                             :262-328) keeps the chunk it peeks at and loses nothing: the flag changes nothing there.               */
    uint8_t* d_out1; size_t cap1;         /* optional caller buffers (16-byte aligned); NULL = context-owned results.  cap must cover the text plus its last line break (a
                                             file that ends without one is trimmed in the result's count, not in the buffer).  When the call fails, what the buffers hold is
                                             unspecified: with caller buffers the text is written before the host has looked at the image's verdict.               */
    uint8_t* d_out2; size_t cap2;
    /* optional chunk index (the .rfq format has none: RfqChunk::read finds chunk c+1 only by parsing chunk c, src/rfqchunk.cpp:161-228,
     * a dependent load per chunk).  A host that has the offsets - it encoded the image (rfq_encode_result.h_chunk_off), or it walked
     * the chunk headers while the image was on its way to the GPU - passes them: h_chunk_off[0 .. n_chunk_off] = byte offset of every
     * chunk in d_rfq and, last, the end of the last chunk.  Every extent is still verified on the device by a full parse of its chunk;
     * a table that does not verify is ignored (the chain is walked instead).  NULL / 0 = walk.                                      */
    const uint64_t* h_chunk_off; uint32_t n_chunk_off; uint32_t reserved3;
} rfq_decode_args;

typedef struct {
    const uint8_t* d_fq1; size_t n1;
    const uint8_t* d_fq2; size_t n2;
    uint32_t n_chunks;
    uint64_t n_reads, n_bases;
    size_t   consumed;                    /* bytes of the image covered by whole chunks                                */
} rfq_decode_result;

/* RfqChunk::read + RfqCodec::decodeChunk + Read::toString for every chunk of the image
 * (src/rfqchunk.cpp:161-228, src/rfqcodec.cpp:826-1260, src/read.cpp:170-172).  Images whose header lacks
 * BIT_ENCODE_QUAL_BY_COL (legacy run-length quality coding, src/rfqcodec.cpp:919-955; v0.5.1 never writes one) decode too. */
RFQ_API int rfq_decode_batch(rfq_ctx* ctx, const rfq_decode_args* args, rfq_decode_result* res);

/* The same image decoded into per-read ARRAYS instead of FASTQ text: row i of each output is the i-th record rfq_decode_batch (split_pe = 0) would
 * write - Repaq::decompress order; for a PE file row 2k is R1 of pair k and row 2k+1 its R2, in its original orientation.  A base row holds exactly
 * the bytes of the record's sequence line (implied N included) or their codes, a quality row the bytes of its quality line minus qual_offset
 * (mod 256); both are padded to row_len.  Names and strand lines are not produced; the NO_LINE_BREAK bits change nothing (rows have no newlines).
 * All three output pointers NULL = a size query: n_rows, n_chunks, max_len and consumed are returned and nothing is decoded.  RFQ_E_NOSPACE (nothing
 * written; the message says what is needed) when row_len < max_len, a row buffer holds fewer than n_rows * row_len bytes or d_lens fewer than
 * n_rows entries.  An image rfq_decode_batch refuses is refused with the same code.  Synchronous: the rows are in place when the call returns.
 * Row buffers with row_len % 16 == 0 and 16-byte alignment are written in whole 16-byte groups; anything else byte by byte. */
#define RFQ_ROWS_ASCII 0        /* base rows hold the FASTQ bytes (A C G T N)          */
#define RFQ_ROWS_CODE  1        /* base rows hold codes: A 0, C 1, G 2, T 3, N 4        */
typedef struct {
    const uint8_t* d_rfq; size_t n;       /* as rfq_decode_args                                                        */
    int32_t  has_header, final;           /* as rfq_decode_args (streaming: consumed = whole chunks)                    */
    const uint64_t* h_chunk_off; uint32_t n_chunk_off;   /* optional chunk index, verified exactly as in rfq_decode_batch */
    uint32_t row_len;                     /* row stride in bytes (>= 1; >= max_len)                                     */
    int32_t  base_mode;                   /* RFQ_ROWS_ASCII / RFQ_ROWS_CODE                                             */
    uint8_t  qual_offset;                 /* quality row byte = quality char - qual_offset (mod 256); 0 = the raw char  */
    uint8_t  pad_base, pad_qual;          /* written at positions >= the read's length                                  */
    uint8_t  reserved;
    uint8_t* d_bases; size_t bases_cap;   /* [n_rows][row_len] device buffer; NULL = no base rows                       */
    uint8_t* d_quals; size_t quals_cap;   /* [n_rows][row_len]; NULL = no quality rows                                  */
    int32_t* d_lens;  size_t lens_cap;    /* [n_rows] read lengths in bytes (4-byte aligned); cap in entries; NULL = not wanted */
} rfq_decode_rows_args;
typedef struct {
    uint64_t n_rows, n_bases;             /* reads (PE: both mates) and the sum of their lengths                         */
    uint32_t n_chunks, max_len;           /* chunks decoded; the longest read                                            */
    size_t   consumed;                    /* bytes of the image covered by whole chunks                                  */
} rfq_decode_rows_result;
RFQ_API int rfq_decode_rows(rfq_ctx* ctx, const rfq_decode_rows_args* args, rfq_decode_rows_result* res);

/* The NAMES of the same rows, in the layout rfq_rows_in takes: name i = the bytes of the first line of record i of rfq_decode_batch (split_pe = 0,
 * bug_compat = 0) - the '@' included, the line break not -, all of them back to back, and n_rows + 1 offsets (name_off[0] = 0, name_off[n_rows] =
 * names_len; 64-bit: a blob may exceed 4 GiB).  Row i here is row i of rfq_decode_rows (a PE file: rows 2k / 2k + 1 are R1 / R2 of pair k); n_rows,
 * n_chunks and consumed are what rfq_decode_rows reports for the same arguments, the streaming contract is the same.  Only the chunk table, the name
 * sections and the coordinate streams of the image are read: none of the base / quality streams.  The text of the STRAND lines is not carried:
 * rfq_rows_in always writes "+", so rows + names re-encode to the same image only for files whose strand lines are "+".
 * size_only = 1: the counts alone, nothing is written.  RFQ_E_NOSPACE (nothing written; the message says "need ...") when a cap is too small,
 * RFQ_E_ARG for a d_name_off that is not 8-byte aligned.  An image rfq_decode_batch refuses in its header or chunk walk is refused with the same
 * code.  Synchronous: names and offsets are in place when the call returns; context-owned results stay valid until the next call on the context. */
typedef struct {
    const uint8_t* d_rfq; size_t n;       /* as rfq_decode_rows_args                                                    */
    int32_t  has_header, final;
    const uint64_t* h_chunk_off; uint32_t n_chunk_off;   /* optional chunk index, verified exactly as in rfq_decode_batch */
    int32_t  size_only;                   /* 1: counts only, nothing written                                            */
    uint8_t*  d_names;    size_t names_cap;   /* caller blob (any alignment) or NULL = context-owned                    */
    uint64_t* d_name_off; size_t off_cap;     /* caller offsets, 8-byte aligned, cap in ENTRIES (>= n_rows + 1), or NULL = context-owned */
} rfq_decode_names_args;
typedef struct {
    const uint8_t*  d_names;    uint64_t names_len;   /* where the blob is (the caller's or the context's)              */
    const uint64_t* d_name_off;           /* [n_rows + 1], name_off[0] = 0, name_off[n_rows] = names_len                */
    uint64_t n_rows; uint32_t n_chunks, max_name;     /* max_name: the longest name line in bytes                       */
    size_t   consumed;
} rfq_decode_names_result;
RFQ_API int rfq_decode_names(rfq_ctx* ctx, const rfq_decode_names_args* args, rfq_decode_names_result* res);

/* The way back: per-read ARRAYS in HBM -> FASTQ text -> .rfq image, nothing on the host.  The row layout is rfq_decode_rows's: row i is record i,
 * `name '\n' bases '\n' '+' '\n' quals '\n'` (the strand line is always "+", every text ends in '\n').  A base row holds the FASTQ bytes or the codes
 * 0..4 (-> A C G T N), a quality row the quality characters minus qual_offset; bytes at positions >= the read's length are never read as data
 * (whatever pad rfq_decode_rows wrote is ignored).  Names are not rows: all name lines back to back ('@' included, no line breaks) and n_rows + 1 offsets.
 * The row buffers may have any alignment; with row_len % 16 == 0 and 16-byte alignment they are loaded in whole 16-byte groups, otherwise at their own
 * alignment - never a byte outside [d_x, d_x + n_rows * row_len).  d_lens is 4-byte, d_name_off 8-byte aligned.  n_rows * row_len and the texts may
 * exceed 4 GiB.
 * Refused, judged on the device before anything is written (the context stays usable): RFQ_E_ARG for a length < 0 or > row_len, for name offsets that
 * decrease or end past names_len, and for an odd n_rows with RFQ_PE_TWO_FILES; RFQ_E_DATA for a length of 0 (an empty sequence line ends the
 * reference's reader, src/fastqreader.cpp:180-191) and for a name of 0 bytes.  Found by the writer itself, RFQ_E_DATA, what the output buffers hold
 * is then unspecified (as with rfq_decode_args's caller buffers): a code above 4, an ASCII base or a quality character (after the offset) outside
 * 0x21..0x7E, '\n' or '\r' in a name.  Everything else (lower-case bases, names over 255 bytes, coordinates) is the encoder's to judge. */
typedef struct {
    uint64_t n_rows;
    uint32_t row_len;                     /* row stride in bytes (>= 1)                                                 */
    int32_t  base_mode;                   /* RFQ_ROWS_ASCII / RFQ_ROWS_CODE                                             */
    uint8_t  qual_offset;                 /* quality char = row byte + qual_offset (mod 256)                            */
    uint8_t  reserved[3];
    const uint8_t* d_bases;               /* [n_rows][row_len]                                                          */
    const uint8_t* d_quals;               /* [n_rows][row_len]                                                          */
    const int32_t* d_lens;                /* [n_rows], 1 <= len <= row_len                                              */
    const uint8_t* d_names; size_t names_len;   /* the name lines, back to back                                         */
    const uint64_t* d_name_off;           /* [n_rows + 1] device offsets into d_names, non-decreasing, last <= names_len */
} rfq_rows_in;
typedef struct {
    const uint8_t* d_fq1; size_t n1;      /* the text (RFQ_PE_TWO_FILES: of the even rows)                              */
    const uint8_t* d_fq2; size_t n2;      /* RFQ_PE_TWO_FILES: the text of the odd rows, else NULL / 0                  */
    uint64_t n_reads, n_bases;
} rfq_rows_text_result;
/* rows -> text.  paired: RFQ_SE and RFQ_PE_INTERLEAVED write one text in row order, RFQ_PE_TWO_FILES rows 2k to text 1 and rows 2k + 1 to text 2.
 * d_out1 / d_out2: caller buffers (16-byte aligned) of cap1 / cap2 bytes; NULL = context-owned buffers, valid until the next call on the context.
 * size_only = 1: n1, n2, n_reads and n_bases are returned and nothing is written.  RFQ_E_NOSPACE (nothing written; the message says what is needed)
 * when a cap is smaller than its text.  Synchronous: the text is in place when the call returns. */
RFQ_API int rfq_rows_to_text(rfq_ctx* ctx, const rfq_rows_in* rows, int32_t paired, uint8_t* d_out1, size_t cap1, uint8_t* d_out2, size_t cap2,
                             int32_t size_only, rfq_rows_text_result* res);
/* rfq_rows_to_text into context-owned text, then rfq_encode_batch(enc) on it: enc->d_fq1 / d_fq2 / n1 / n2 must be NULL / 0 (the call fills them in), and
 * final or flush_all must be set - a rows batch is always encoded whole, there is no text to report `consumed` against (RFQ_E_ARG otherwise).  paired,
 * chunk_bases, emit_header, d_out / out_cap, the line-break fields and the header state behave as in rfq_encode_batch; several row batches make one
 * file: the first with emit_header = 1, flush_all = 1, the last with final = 1.  A refusal of the rows leaves the encoder unrun. */
RFQ_API int rfq_encode_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_encode_args* enc, rfq_encode_result* res);

/* The front door of the row interface: FASTQ TEXT in HBM -> per-read rows, lengths and names, without an image in between.  Row i is the i-th record the
 * reference's reader hands the codec for this text - exactly the records rfq_encode_batch would encode, by the same line index and the same rules: line ends
 * '\n', '\r' and "\r\n", a single blank line is swallowed, the reader stops for good at the first empty line (input_ended), a trailing partial record is dropped,
 * RFQ_PE_TWO_FILES stops with the shorter file (rows 2k / 2k + 1 = record k of file 1 / file 2), RFQ_PE_INTERLEAVED gives an even number of rows in text order.
 * The bytes are the text's own, in their original orientation: a base row in ASCII mode holds the sequence line verbatim (lower case, IUPAC codes and all), in
 * code mode A C G T N -> 0..4 and any other byte is RFQ_E_DATA (the message names the first such row; what the buffers hold is then unspecified); a quality row
 * holds the quality characters minus qual_offset (mod 256), of a quality line longer than its sequence line the first `length` characters (what the codec keeps);
 * positions >= the read's length hold pad_*; lens[i] = bytes of the sequence line.  A quality line SHORTER than its sequence line is RFQ_E_UNPINNED, as in the
 * encoder.  Name i = the first line of record i, '@' included, without its line break (no '\r' either), in rfq_rows_in's layout: name_off[0] = 0,
 * name_off[n_rows] = names_len.  The text of the STRAND lines is not carried, like everywhere in the row interface: rows + names re-encode (rfq_encode_rows) to
 * the text's image only for files whose strand lines are "+".
 * All five output pointers NULL = a size query: every field of the result is filled, nothing is written (row_len is not looked at).  An output that is NULL is
 * not produced.  RFQ_E_NOSPACE (nothing written; the message says "need ...") when row_len < max_len or a cap is too small; RFQ_E_ARG for a bad paired /
 * base_mode, row_len == 0, a d_lens that is not 4-byte or a d_name_off that is not 8-byte aligned, a d_fq2 without RFQ_PE_TWO_FILES.  After any refusal the
 * context stays usable.
 * Streaming: one call indexes with 32-bit offsets, so it takes of each stream at most the encoder's slice (3 GiB; RFQ_SLICE_BYTES sets a small one) - what lies
 * beyond is treated as if final = 0.  consumed1 / consumed2 say where the next call starts, in the caller's bytes (also when the text was normalised); the rows
 * of consecutive calls, concatenated by the caller, are the one-shot rows.  With final = 0 only whole records are taken (an unterminated last line is not a
 * line).  n_rows * row_len may exceed 4 GiB.  Synchronous on the context's stream, like rfq_decode_rows. */
typedef struct {
    const uint8_t* d_fq1; size_t n1;      /* as rfq_encode_args: any alignment, up to 15 bytes in front may be read */
    const uint8_t* d_fq2; size_t n2;      /* RFQ_PE_TWO_FILES only */
    int32_t  paired;                      /* RFQ_SE / RFQ_PE_TWO_FILES / RFQ_PE_INTERLEAVED */
    int32_t  final;                       /* 1: end of the input (an unterminated last line is a line); 0: whole records only, see consumed */
    uint64_t file_off1, file_off2;        /* offset of this text in its file: the reader's 1 MiB block rule, as in rfq_encode_args */
    uint32_t row_len; int32_t base_mode;  /* as rfq_decode_rows_args */
    uint8_t  qual_offset, pad_base, pad_qual, reserved;
    uint8_t* d_bases; size_t bases_cap;   /* [n_rows][row_len] or NULL */
    uint8_t* d_quals; size_t quals_cap;   /* [n_rows][row_len] or NULL */
    int32_t* d_lens;  size_t lens_cap;    /* [n_rows] (entries) or NULL */
    uint8_t* d_names; size_t names_cap;   /* blob, any alignment, or NULL */
    uint64_t* d_name_off; size_t off_cap; /* [n_rows + 1] (entries), 8-byte aligned, or NULL */
} rfq_text_rows_args;
typedef struct {
    uint64_t n_rows, n_bases, names_len;
    uint32_t max_len, max_name;
    size_t   consumed1, consumed2;        /* bytes of each stream covered by the rows */
    int32_t  input_ended, reserved;       /* as rfq_encode_result */
} rfq_text_rows_result;
RFQ_API int rfq_text_rows(rfq_ctx* ctx, const rfq_text_rows_args* args, rfq_text_rows_result* res);

/* The step in the middle of the row interface: rows (rfq_decode_rows / rfq_text_rows + their names) -> the rows a caller KEEPS, each TRIMMED to a window, compacted,
 * with their lengths, names and name offsets - what rfq_encode_rows / rfq_rows_to_text take.  The caller decides (a mask, a window per row - its own code over the
 * row arrays); this call moves the bytes, nothing on the host.
 * Kept rows: output row j is the j-th kept input row, in input order.  Its bytes are input bytes [start, start + len) of the base and of the quality row, unchanged
 * - no code / ASCII or quality-offset transform: base_mode and qual_offset of `rows` are not looked at -, positions >= the new length hold pad_*, lens[j] is the window
 * length, its name is the whole input name; name_off[0] = 0, name_off[n_out] = names_len.
 * Why a row is dropped, counted once, in this order: dropped_mask - keep[i] == 0; dropped_short - its window is shorter than min_len; dropped_mate (pairs only) - the
 * row would stand, its mate (row i ^ 1) does not.  n_in == n_rows + the three.
 * rows->d_name_off == NULL means rows without names: d_names / d_name_off of the arguments must then be NULL too (RFQ_E_ARG), names_len and max_name are 0.
 * All five output pointers NULL = a size query: the whole result is filled, nothing is written (row_len is not looked at).  An output that is NULL is not produced
 * (rows->d_bases / d_quals may be NULL with theirs).  RFQ_E_NOSPACE (nothing written; the message says "need ...") when row_len < max_len or a cap is too small.
 * RFQ_E_ARG, judged on the host: an odd n_rows with pairs, row_len == 0 on a call that is not a size query, a d_lens / d_start / d_len that is not 4-byte or a
 * d_name_off that is not 8-byte aligned, an output buffer that overlaps an input buffer (the byte ranges are compared - of an output the bytes a call can write: its
 * cap, at most n_rows rows; selection in place is not offered).  RFQ_E_ARG, judged on the device before anything is written, the message names the first such row:
 * lens[i] < 0 or > rows->row_len; start < 0, len < 0 or start + len > lens[i] (formed in 64 bits); name offsets that decrease or end past names_len.  ALL rows are
 * judged, kept or not.  After any refusal the context stays usable.
 * The row buffers may have any alignment, in and out: with row_len % 16 == 0 and 16-byte alignment they are loaded / stored in whole 16-byte groups, otherwise at
 * their own alignment - never a byte outside [d_x, d_x + n * row_len) of either side.  n_rows * row_len and the blob may exceed 4 GiB (n_rows < 2^32 - 16).
 * Synchronous on the context's stream, like rfq_text_rows; stage times through rfq_last_timings (select:judge, select:tables, select:rows, select:names).
 *
 * A TAG of the read's own bases in the kept names (args->tag, a HOST struct; NULL: names are kept whole, everything above) - UMI extraction in the manner of fastp's
 * --umi and umi_tools extract: the bases are cut off through d_start, the tag carries them in the name.
 * part(i) is the d_tag_len[i] bytes of base row i from d_tag_start[i], as text: with rows->base_mode == RFQ_ROWS_CODE the codes 0 .. 4 become A C G T N, with
 * RFQ_ROWS_ASCII the bytes stand as they lie (lower case and N survive).  base_mode is looked at only when tag is given.  The part may lie anywhere in the read:
 * d_start / d_len are independent of it.  The unit's tag T: pairs = 0 - T(i) = part(i); pairs = 1 - both rows of pair u get T(u) = part(2u), then `join` if both parts
 * have bytes, then part(2u + 1) (a kept pair's mate is kept too, so both rows are rows of this call).  The text inserted is X = sep, then prefix and join if
 * prefix_len > 0, then T: 81 bytes at most.  If T is empty nothing is inserted at all and the name is the input name.  Where: RFQ_TAG_AT_SPACE - in front of the
 * first 0x20 byte of the name (no other byte counts as a space), a name without one: at its end; RFQ_TAG_AT_END - at its end; a name of 0 bytes takes X at offset 0.
 * names_len, max_name and name_off count the tags; the size query, RFQ_E_NOSPACE and "an output that is NULL is not produced" are unchanged.
 * RFQ_E_ARG, judged on the host: tag with rows without names; d_tag_start or d_tag_len NULL (with n_rows > 0, like rows->d_bases below) or not 4-byte aligned; prefix_len > RFQ_TAG_PREFIX_MAX, h_prefix NULL
 * with prefix_len > 0; sep, join or a prefix byte outside 0x21..0x7E; at other than the two; a bad base_mode; rows->d_bases NULL; a tag array that overlaps an output.
 * Judged on the device before anything is written, ALL rows, kept or not, the message names the first such row: RFQ_E_ARG - tag_start < 0, tag_len < 0, tag_len >
 * RFQ_TAG_PART_MAX, tag_start + tag_len > lens[i] (formed in 64 bits); RFQ_E_DATA - a part byte that is a code above 4 / an ASCII byte outside 0x21..0x7E.
 * RFQ_E_ARG, behind the judge: a KEPT name of 4 GiB or more (the plan holds a name's length and the place in 32 bits); the plain call takes such a name.
 * Stage times: select:tagplan (where X goes, X rendered once per output row into scratch of the context's) in front of select:names.  RFQ_TAG=general takes the
 * other formulation: a thread per output name, byte by byte, no plan.
 * NOT offered: UMIs read out of the name line (fastp's index1 / index2 / per_index), tags in rfq_group_rows / rfq_merge_rows, UMI quality filters, parts of more than
 * RFQ_TAG_PART_MAX bases, UMI-aware near-duplicate removal (an inline UMI is part of rfq_dedup_rows' key when dedup runs before this step). */
#define RFQ_TAG_PART_MAX   32             /* bases one row gives                                                        */
#define RFQ_TAG_PREFIX_MAX 14
#define RFQ_TAG_AT_SPACE   0              /* in front of the first 0x20 byte of the name; a name without one: at its end (fastp) */
#define RFQ_TAG_AT_END     1
typedef struct {
    const int32_t* d_tag_start;           /* [n_rows] first base of row i's part                                        */
    const int32_t* d_tag_len;             /* [n_rows] its bases, 0 .. RFQ_TAG_PART_MAX; 0: row i gives no part          */
    const uint8_t* h_prefix;              /* HOST bytes or NULL                                                         */
    uint32_t prefix_len;                  /* 0 .. RFQ_TAG_PREFIX_MAX                                                    */
    uint8_t  sep, join, at, reserved;
} rfq_name_tag;
typedef struct {
    const uint8_t* d_keep;                /* [n_rows] bytes, non-zero = keep (a torch.bool tensor as it lies); NULL = every row */
    const int32_t* d_start;               /* [n_rows] first base kept of row i; NULL = 0                                */
    const int32_t* d_len;                 /* [n_rows] bases kept from there; NULL = to the end of the read (lens[i] - start[i]) */
    int32_t  pairs;                       /* 1: rows 2k / 2k + 1 stand or fall together (n_rows must be even)           */
    uint32_t min_len;                     /* a row whose window is shorter is dropped; 0 lets empty rows through (the encoder refuses them later) */
    uint32_t row_len;                     /* OUTPUT stride (>= 1, >= the longest kept window; may differ from rows->row_len) */
    uint8_t  pad_base, pad_qual, reserved[2];
    uint8_t* d_bases; size_t bases_cap;   /* [n_out][row_len] or NULL                                                   */
    uint8_t* d_quals; size_t quals_cap;   /* [n_out][row_len] or NULL                                                   */
    int32_t* d_lens;  size_t lens_cap;    /* [n_out] (entries) or NULL                                                  */
    uint8_t* d_names; size_t names_cap;   /* blob, any alignment, or NULL                                               */
    uint64_t* d_name_off; size_t off_cap; /* [n_out + 1] (entries), 8-byte aligned, or NULL                             */
    const rfq_name_tag* tag;              /* HOST struct, or NULL: names are kept whole (today's call)                  */
} rfq_select_rows_args;
typedef struct {
    uint64_t n_rows, n_bases, names_len;  /* of the OUTPUT                                                              */
    uint32_t max_len, max_name;
    uint64_t n_in, dropped_mask, dropped_short, dropped_mate;   /* n_in == n_rows + the three                           */
} rfq_select_rows_result;
RFQ_API int rfq_select_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_select_rows_args* args, rfq_select_rows_result* res);

/* rfq_select_rows with the kept rows GROUPED by an integer bin per unit, in ONE pass over the rows: a stable partition - the reads of one sample next to each other
 * (d_bin = rfq_demux_rows' d_sample as it lies), rows by length bin, by rfq_dedup_rows' representative, by rfq_screen_rows' verdict.  A unit is a row, with pairs the
 * rows 2k / 2k + 1; d_bin has one entry per unit.  T = n_bins + rest bins in all, 1 <= n_bins, T <= 65536, rest 0 or 1.  A unit with 0 <= bin < n_bins belongs to
 * that bin; one with bin < 0 to bin n_bins with rest = 1, with rest = 0 it is dropped with all its rows; bin >= n_bins is RFQ_E_ARG.
 * Who stays is otherwise rfq_select_rows' rule, unchanged: the mask, the windows and their validation, min_len, the pair rule.  Why a row is dropped, counted once,
 * in this order: dropped_mask - keep[i] == 0; dropped_bin - its unit's bin < 0 with rest = 0; dropped_short - its window is shorter than min_len; dropped_mate (pairs
 * only) - the row would stand, its mate does not.  n_in == n_rows + the four.
 * Order: the output rows are the kept rows sorted by (bin, input row) - a stable sort; the rows of a pair stay adjacent, R1 first.  d_bin_off[b], b in [0, T], is the
 * first output ROW of bin b (empty bins included), d_bin_off[T] == n_rows of the result.  lens, name_off and the blob are in output order, so the names of bin b
 * are the blob bytes [name_off[bin_off[b]], name_off[bin_off[b + 1]]).
 * The contract in one sentence: for every bin b the output rows [bin_off[b], bin_off[b + 1]) are byte for byte what rfq_select_rows writes with the same d_start /
 * d_len / pairs / min_len / row_len / pads and the mask "keep AND bin == b" spread to the rows of a unit - their lengths, their names and their name offsets less
 * the first included.  n_bins_used: the bins that hold a row.
 * rows->d_name_off == NULL means rows without names: d_names / d_name_off of the arguments must then be NULL too (RFQ_E_ARG), names_len and max_name are 0.
 * All SIX output pointers NULL (d_bin_off with the five of rfq_select_rows) = a size query: the whole result is filled, nothing is written.  An output that is NULL is
 * not produced; d_bin_off alone gives the rows per bin without moving a row (row_len is looked at only where one of the other five is asked for).  RFQ_E_NOSPACE
 * (nothing written; the message says "need ...") when row_len < max_len, a cap is too small or bin_cap < T + 1.
 * RFQ_E_ARG, judged on the host: what rfq_select_rows refuses (an odd n_rows with pairs, row_len == 0 where rows are written, misaligned d_lens / d_start / d_len /
 * d_name_off, an output that overlaps an input); d_bin == NULL with rows; n_bins == 0; T > 65536; rest not 0 or 1; a d_bin that is not 4-byte or a d_bin_off that is
 * not 8-byte aligned; an output that overlaps d_bin, d_bin_off overlapping an input (byte ranges; of d_bin_off min(bin_cap, T + 1) entries).  RFQ_E_ARG, judged on the
 * device before anything is written: rfq_select_rows' (the message names the first such row) and a bin >= n_bins (the message names the first such UNIT).  ALL rows
 * and units are judged, kept or not.  After any refusal the context stays usable.
 * The row buffers may have any alignment, in and out; n_rows * row_len and the blob may exceed 4 GiB (n_rows < 2^32 - 16).  The same call writes the same bytes: no
 * atomic decides where a row goes.  Scratch is O(units) and the context's own.  Synchronous on the context's stream; stage times through rfq_last_timings
 * (group:judge, group:rank, group:tables, group:rows, group:names). */
typedef struct {
    const uint8_t* d_keep;                /* [n_rows] bytes, non-zero = keep; NULL = every row                          */
    const int32_t* d_start;               /* [n_rows] first base kept of row i; NULL = 0                                */
    const int32_t* d_len;                 /* [n_rows] bases kept from there; NULL = to the end of the read              */
    int32_t  pairs;                       /* 1: rows 2k / 2k + 1 are one unit (n_rows must be even)                     */
    uint32_t min_len;                     /* a row whose window is shorter is dropped                                   */
    const int32_t* d_bin;                 /* [units] the unit's bin: 0 .. n_bins - 1; < 0: the rest bin, or dropped     */
    uint32_t n_bins;                      /* >= 1; n_bins + rest <= 65536                                               */
    int32_t  rest;                        /* 1: units with bin < 0 make bin n_bins; 0: they are dropped                 */
    uint64_t* d_bin_off; size_t bin_cap;  /* [n_bins + rest + 1] (entries) first output row of each bin, 8-byte aligned, or NULL */
    uint32_t row_len;                     /* OUTPUT stride (>= 1, >= the longest kept window)                           */
    uint8_t  pad_base, pad_qual, reserved[2];
    uint8_t* d_bases; size_t bases_cap;   /* [n_out][row_len] or NULL                                                   */
    uint8_t* d_quals; size_t quals_cap;   /* [n_out][row_len] or NULL                                                   */
    int32_t* d_lens;  size_t lens_cap;    /* [n_out] (entries) or NULL                                                  */
    uint8_t* d_names; size_t names_cap;   /* blob, any alignment, or NULL                                               */
    uint64_t* d_name_off; size_t off_cap; /* [n_out + 1] (entries), 8-byte aligned, or NULL                             */
} rfq_group_rows_args;
typedef struct {
    uint64_t n_rows, n_bases, names_len;  /* of the OUTPUT                                                              */
    uint32_t max_len, max_name;
    uint64_t n_in, dropped_mask, dropped_short, dropped_mate;
    uint64_t dropped_bin;                 /* n_in == n_rows + the four                                                  */
    uint32_t n_bins_used, reserved;       /* bins that hold a row                                                       */
} rfq_group_rows_result;
RFQ_API int rfq_group_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_group_rows_args* args, rfq_group_rows_result* res);

/* The step that DECIDES, in front of rfq_select_rows: rows -> per row a keep byte, a window (start, len), a reason byte and four metrics - exactly the d_keep /
 * d_start / d_len arrays rfq_select_rows takes - and one QC summary of the batch.  Quality trimming and filtering by integer rules of this project's own
 * (a sliding window in the manner of Trimmomatic, filters in the manner of fastp; no parity with either is claimed).  No float anywhere, products in 64 bits.
 * A quality row byte IS the score (rows hold "quality character minus qual_offset"; rows->qual_offset is not looked at).  rows->base_mode says what a base
 * byte is: N is code 4 or 'N' / 'n', G is code 2 or 'G' / 'g'.  Names are not looked at (d_names / d_name_off may be NULL).
 * Per row with l = lens[i], bases b, scores q and S(p, w) = q[p] + ... + q[p + w - 1], in this order; a step that is off, or whose window [a, e) is already
 * empty, is skipped:
 *   a = min(trim_front, l);  e = max(a, l - min(trim_tail, l))
 *   poly_g > 0:      r = length of the run of G that ends at e - 1 inside [a, e);  r >= poly_g: e -= r
 *   RFQ_CUT_FRONT:   w = min(cut_window, e - a);  p = the smallest p in [a, e - w] with S(p, w) >= cut_mean_q * w;  none: e = a;  else a = p
 *   RFQ_CUT_RIGHT:   w = min(cut_window, e - a);  p = the smallest p in [a, e - w] with S(p, w) <  cut_mean_q * w;  found: e = p
 *   RFQ_CUT_TAIL:    w = min(cut_window, e - a);  p = the largest  p in [a, e - w] with S(p, w) >= cut_mean_q * w;  none: e = a;  else e = p + w
 *   max_len > 0:     e = min(e, a + max_len)
 *   start = a;  len = n = e - a
 * Metrics of the final window: qsum = S(a, n); n_cnt = its N; lowq = its q < qual_q (0 with qual_q == 0); trans = the j in [a, e - 1) with b[j] != b[j + 1]
 * (a byte compare).  All reasons are evaluated and ORed into why; keep = (why == 0):
 *   RFQ_WHY_SHORT    n < min_len                        RFQ_WHY_N        max_n >= 0 && n_cnt > max_n
 *   RFQ_WHY_MEANQ    qsum < min_mean_q * n              RFQ_WHY_LOWQ     qual_q > 0 && lowq * 100 > max_lowq_pct * n
 *   RFQ_WHY_COMPLEX  n > 1 && trans * 100 < min_complexity_pct * (n - 1)
 * The pair rule is rfq_select_rows's (pairs = 1): this call judges each row on its own.
 * Every output is [n_rows] entries (d_metrics [n_rows][4]: qsum, n_cnt, lowq, trans); an output that is NULL is not produced; the result is filled also when all
 * five are NULL.  The *_in fields are taken over the whole reads [0, l), the *_out fields over the windows of the kept rows; q20 / q30: scores >= 20 / >= 30.
 * RFQ_E_ARG, judged on the host: unknown cut_flags bits, a cut flag with cut_window outside 1 .. 1000, a percentage above 100, a bad base_mode, row_len == 0 with
 * rows, d_quals == NULL with a quality criterion set (a cut flag, min_mean_q, qual_q), d_bases == NULL with poly_g, max_n >= 0 or min_complexity_pct set, a d_lens /
 * d_start / d_len / d_metrics that is not 4-byte aligned, an output that overlaps an input.  RFQ_E_ARG, judged on the device, the message names the first such
 * row: lens[i] < 0 or > row_len - what the outputs hold is then unspecified; nothing outside the row buffers is read for such a row.  After any refusal the context
 * stays usable.
 * The row buffers may have any alignment: with row_len % 16 == 0 and 16-byte alignment they are loaded in whole 16-byte groups, otherwise at their own alignment -
 * never a byte outside [d_x, d_x + n_rows * row_len).  n_rows * row_len may exceed 4 GiB (n_rows < 2^31).  Every sum is an integer: the same call gives the same
 * bytes.  Synchronous on the context's stream; stage time through rfq_last_timings (judge:rows). */
#define RFQ_CUT_FRONT   1u
#define RFQ_CUT_RIGHT   2u
#define RFQ_CUT_TAIL    4u
#define RFQ_WHY_SHORT   1u
#define RFQ_WHY_N       2u
#define RFQ_WHY_MEANQ   4u
#define RFQ_WHY_LOWQ    8u
#define RFQ_WHY_COMPLEX 16u
typedef struct {
    uint32_t trim_front, trim_tail;       /* bases taken off either end first                                           */
    uint32_t poly_g;                      /* > 0: a trailing run of at least that many G is cut                         */
    uint32_t cut_flags;                   /* RFQ_CUT_FRONT | RFQ_CUT_RIGHT | RFQ_CUT_TAIL                               */
    uint32_t cut_window, cut_mean_q;      /* 1 .. 1000 with a cut flag; a window is good when its sum >= cut_mean_q * w */
    uint32_t max_len;                     /* > 0: the window is cut to that many bases                                  */
    uint32_t min_len;
    int32_t  max_n;                       /* < 0: off                                                                   */
    uint32_t min_mean_q, qual_q, max_lowq_pct, min_complexity_pct;
    uint32_t reserved;
    uint8_t*  d_keep;                     /* [n_rows] 1 / 0, or NULL                                                    */
    int32_t*  d_start;                    /* [n_rows] or NULL                                                           */
    int32_t*  d_len;                      /* [n_rows] or NULL                                                           */
    uint8_t*  d_why;                      /* [n_rows] RFQ_WHY_* bits, or NULL                                           */
    uint32_t* d_metrics;                  /* [n_rows][4] qsum, n_cnt, lowq, trans, or NULL                              */
} rfq_judge_rows_args;
typedef struct {
    uint64_t n_rows, n_kept;
    uint64_t why_short, why_n, why_meanq, why_lowq, why_complex;   /* rows with that bit set                            */
    uint64_t bases_in, qsum_in, q20_in, q30_in;                    /* over the whole reads                              */
    uint64_t bases_out, qsum_out, q20_out, q30_out;                /* over the windows of the kept rows                 */
} rfq_judge_rows_result;
RFQ_API int rfq_judge_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_judge_rows_args* args, rfq_judge_rows_result* res);

/* Adapter removal, in front of rfq_judge_rows: rows -> per row the length that is left and the detector that cut it, per pair the insert size and the mismatch
 * count of the overlap found, per batch a summary and an insert-size histogram.  Like rfq_judge_rows it DECIDES and moves no bytes: d_len is what rfq_select_rows
 * takes as d_len (start 0) and, never greater than lens[i] and possibly 0, also valid as the d_lens of a later rfq_judge_rows - adapter -> judge on the shortened
 * lengths -> select, all on the GPU.  Integer rules of this project's own (in the manner of fastp's overlap analysis and adapter match; no parity with fastp is
 * claimed).  No float anywhere, products in 64 bits; the same call gives the same bytes.  Quality rows and names are not looked at (d_quals, d_names, d_name_off
 * may be NULL).
 * Base classes.  rows->base_mode says what a base byte is: in code mode 0 1 2 3 are A C G T, in ASCII mode 'A' 'C' 'G' 'T' in either case; every other byte (code 4
 * and above, N, IUPAC letters) is OTHER.  The complement swaps A with T and C with G and leaves other as other.  Two positions AGREE when both are in A C G T and
 * equal; a position that is other never agrees.  Only positions < lens[i] of a row are data: what lies behind a read never influences a result.
 * Pair overlap (pairs = 1; rows 2k / 2k + 1 are R1 / R2 of pair k).  x = R1, l1 bases; y = the reverse complement of R2, l2 bases: y[j] = comp(r2[l2 - 1 - j]).
 * A shift d aligns y[j] with x[j + d]; the compared positions are j in [max(0, -d), min(l2, l1 - d)), ov(d) is their number and diff(d) the number of them that do
 * not agree.  d is ACCEPTABLE when ov(d) >= min_overlap, diff(d) <= max_diff and diff(d) * 100 <= max_diff_pct * ov(d).  Shifts are tried in this order: first
 * d = 0, 1, ..., l1 - min_overlap, then d = -1, -2, ..., -(l2 - min_overlap) (a range whose end lies below its start is empty); the first acceptable shift wins - no
 * shift is skipped by an early-exit heuristic, the full count decides.  Found: insert = d + l2, diff = diff(d), cut_o(R1) = min(l1, insert), cut_o(R2) =
 * min(l2, insert).  Not found: insert = -1, diff = 0, cut_o = the row's length.
 * Adapter match, per row: without pairs every row uses adapter 1, with pairs even rows adapter 1 and odd rows adapter 2; either may be off.  For a row of l bases
 * and an adapter A of m bases, p in [0, l): c = min(m, l - p), diff_a(p) = the number of j < c for which row[p + j] does not agree with A[j]; p is acceptable when
 * c >= adapter_min and either adapter_mm_per == 0 and diff_a(p) == 0, or adapter_mm_per > 0 and diff_a(p) * adapter_mm_per <= c.  cut_a = the smallest acceptable p,
 * or l.  The match runs over the whole read, independent of the overlap's verdict.
 * Per row: len = min(cut_o, cut_a); how has RFQ_CUT_BY_OVERLAP set when cut_o < l and RFQ_CUT_BY_ADAPTER when cut_a < l (both may be set).
 * The histogram is zeroed, then filled: bin b < hist_len - 1 counts the found pairs with insert == b, the last bin those with insert >= hist_len - 1; pairs without
 * an overlap are not counted.  An output that is NULL is not produced; the result is filled also when every output is NULL.  rows_cut: rows with len < l.
 * RFQ_E_ARG, judged on the host: an odd n_rows with pairs; with pairs min_overlap == 0 or max_diff_pct > 100; an adapter longer than 64 bases or with a byte other
 * than ACGTacgt; h_adapter2, d_insert, d_diff or d_insert_hist without pairs; adapter_min outside 1 .. 64 with an adapter; hist_len == 0 with a histogram pointer or
 * hist_len > 65536; d_bases == NULL or row_len == 0 with rows; a bad base_mode; a d_lens / d_len / d_insert / d_diff that is not 4-byte or a d_insert_hist that is
 * not 8-byte aligned; an output that overlaps an input (byte ranges are compared).  Neither pairs nor an adapter is NOT an error: every row keeps its length.
 * RFQ_E_ARG, judged on the device, the message names the first such row: lens[i] < 0 or > row_len - what the outputs hold is then unspecified; nothing outside the
 * row buffers is read for such a row.  After any refusal the context stays usable.
 * The row buffer may have any alignment, on rfq_judge_rows' terms - never a byte outside [d_bases, d_bases + n_rows * row_len).  n_rows * row_len may exceed 4 GiB
 * (n_rows < 2^31).  Rows of up to 1024 bytes are searched as bit planes (64 positions per word); longer ones (and every one with RFQ_ADAPTER=general) byte by byte,
 * a lane per shift: the search is quadratic in the read length, and slow on very long rows.  Synchronous on the context's stream; stage time through
 * rfq_last_timings (adapter:rows). */
#define RFQ_CUT_BY_OVERLAP 1u
#define RFQ_CUT_BY_ADAPTER 2u
typedef struct {
    int32_t  pairs;                       /* 1: overlap search on, n_rows must be even                                  */
    uint32_t min_overlap, max_diff, max_diff_pct;      /* pairs: min_overlap >= 1, max_diff_pct <= 100                  */
    const uint8_t* h_adapter1; uint32_t adapter1_len;  /* HOST bytes, A C G T in either case, 1 .. 64; NULL / 0 = off   */
    const uint8_t* h_adapter2; uint32_t adapter2_len;  /* pairs only (odd rows)                                         */
    uint32_t adapter_min, adapter_mm_per; /* with an adapter: adapter_min in 1 .. 64                                    */
    uint32_t hist_len;                    /* entries of d_insert_hist, <= 65536                                         */
    int32_t*  d_len;                      /* [n_rows] or NULL                                                           */
    uint8_t*  d_how;                      /* [n_rows] RFQ_CUT_BY_* bits, or NULL                                        */
    int32_t*  d_insert;                   /* [n_rows / 2] insert or -1, or NULL; pairs only                             */
    int32_t*  d_diff;                     /* [n_rows / 2], or NULL; pairs only                                          */
    uint64_t* d_insert_hist;              /* [hist_len], 8-byte aligned, or NULL; pairs only                            */
} rfq_adapter_rows_args;
typedef struct {
    uint64_t n_rows, n_pairs, pairs_found;
    uint64_t rows_cut, rows_cut_overlap, rows_cut_adapter;   /* len < l; the how bits                                   */
    uint64_t bases_in, bases_out;
} rfq_adapter_rows_result;
RFQ_API int rfq_adapter_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_adapter_rows_args* args, rfq_adapter_rows_result* res);

/* Merging, behind rfq_adapter_rows: every pair with an insert size becomes ONE row of `insert` bases - the fragment both mates were read from, R1 from its front, the
 * reverse complement of R2 from its back, the consensus of the two where they overlap - under R1's name (in the manner of fastp --merge, PEAR, BBMerge).  Like
 * rfq_select_rows it moves bytes and takes no decision about the alignment: d_insert says which pairs merge and at which shift.  Integer rules of this project's own;
 * no parity with any tool is claimed.  No float anywhere; the same call gives the same bytes.  A quality row byte IS the score (rows->qual_offset is not looked at).
 * Inputs.  Rows 2k / 2k + 1 are R1 / R2 of pair k, l1 / l2 their lengths, r1, q1, r2, q2 their bases and scores; ins = d_insert[k].  A pair is merged when ins >= 0
 * (rfq_adapter_rows leaves -1 for a pair without an overlap; a caller narrows further by writing -1 itself).  Output row j is the j-th merged pair, in input order:
 * its length is ins, its name the whole name of row 2k (R2's name is dropped); name_off[0] = 0 and name_off[n_out] = names_len.
 * Fragment coordinates, p in [0, ins).  R1 covers p < min(l1, ins) with (r1[p], q1[p]).  R2 covers p >= ins - l2 with (comp(r2[i]), q2[i]), i = ins - 1 - p.  comp is
 * rfq_adapter_rows' complement as a byte map: in code mode it swaps 0 with 3 and 1 with 2, in ASCII mode A with T, C with G, a with t and c with g; every other
 * byte is itself.  This is rfq_adapter_rows' alignment with d = ins - l2: y[j] = comp(r2[l2 - 1 - j]) lies at x[j + d].  The same insert stays valid for lengths cut
 * to min(l, insert): of a mate longer than the insert only its first insert bases are looked at (R1's tail is left out; R2's index i = ins - 1 - p is below ins), so
 * the merged row is the same.  It does NOT stay valid for lengths cut further by the adapter match (rfq_adapter_rows' d_len where RFQ_CUT_BY_ADAPTER is set): merge
 * with the lengths the insert was found on, or with min(l, insert).
 * A position one mate covers takes that mate's base and score.  A position both cover - classes and AGREE are rfq_adapter_rows' definitions, b2 = comp(r2[i]):
 *   1. they agree:                                   the base is r1[p] (R1's byte, in its case), the score max(q1, q2)
 *   2. exactly one of them is in A C G T:            that one wins, with its own score
 *   3. otherwise (two different A C G T, two others): q1 >= q2: r1[p] with score q1 - q2; else b2 with score q2 - q1
 * Positions >= ins of an output row hold pad_base / pad_qual.
 * Sizes.  All five outputs NULL = a size query: the whole result is filled, nothing is written.  An output that is NULL is not produced.  RFQ_E_NOSPACE with a
 * "need ..." message, and nothing written, when row_len < max_len or a cap is too small.  Rows without names: rows->d_name_off == NULL, and then d_names /
 * d_name_off must be NULL.  Either row output needs BOTH rows->d_bases and rows->d_quals: the rule looks at the bases and the scores.
 * RFQ_E_ARG, judged on the host: an odd n_rows; d_insert == NULL with rows; a d_insert, d_lens or rows->d_lens that is not 4-byte aligned; a d_name_off that is not
 * 8-byte aligned; row_len == 0 on a call that writes; a bad base_mode; rows->d_bases or rows->d_quals NULL with a row output wanted; an output that overlaps an
 * input (byte ranges, as rfq_select_rows compares them).  RFQ_E_ARG, judged on the device before anything is written, the message names the first such row or pair
 * - ALL pairs are judged, merged or not: lens[i] < 0 or > rows->row_len; for a pair with ins >= 0: l1 == 0, l2 == 0, ins == 0 or ins > l1 + l2 - 1, that is, no
 * position that both mates cover; name offsets that decrease or end past names_len.  After any refusal the context stays usable.
 * The row buffers may have any alignment on either side - never a byte outside [d_x, d_x + n * row_len).  n_rows * row_len may exceed 4 GiB.  The default kernel
 * takes a 16-byte group of an output row per lane (R2's bytes in one load, reversed and complemented in registers, the rule as byte masks); RFQ_MERGE=general takes
 * a lane per output byte with the rule as plain branches - the same bytes.  Synchronous on the context's stream; stage times through rfq_last_timings (merge:judge,
 * merge:tables, merge:rows, merge:names). */
typedef struct {
    const int32_t* d_insert;              /* [n_rows / 2]: the pair's insert size (rfq_adapter_rows' d_insert); < 0 = the pair is not merged */
    uint32_t row_len;                     /* OUTPUT stride (>= 1, >= the longest merged read; may exceed rows->row_len: up to 2 * row_len - 1) */
    uint8_t  pad_base, pad_qual, reserved[2];
    uint8_t* d_bases; size_t bases_cap;   /* [n_out][row_len] or NULL                                                   */
    uint8_t* d_quals; size_t quals_cap;   /* [n_out][row_len] or NULL                                                   */
    int32_t* d_lens;  size_t lens_cap;    /* [n_out] (entries) or NULL                                                  */
    uint8_t* d_names; size_t names_cap;   /* blob, any alignment, or NULL                                               */
    uint64_t* d_name_off; size_t off_cap; /* [n_out + 1] (entries), 8-byte aligned, or NULL                             */
} rfq_merge_rows_args;
typedef struct {
    uint64_t n_rows, n_bases, names_len;  /* of the OUTPUT: n_rows = merged pairs                                       */
    uint32_t max_len, max_name;
    uint64_t n_pairs, overlap_bases;      /* pairs in; sum over merged pairs of the positions both mates cover          */
} rfq_merge_rows_result;
RFQ_API int rfq_merge_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_merge_rows_args* args, rfq_merge_rows_result* res);

/* Duplicate removal, between rfq_judge_rows and rfq_select_rows: rows -> a keep byte per row that leaves ONE unit of every class of identical units (in the manner of
 * fastp --dedup and clumpify dedupe; exact byte equality, no parity with either is claimed), the representative and the size of every class, a class-size histogram
 * and a summary.  Like rfq_judge_rows it DECIDES and moves no bytes: d_keep is exactly rfq_select_rows' d_keep - adapter -> judge -> dedup -> select -> encode, all on
 * the GPU.  It is the one step of the family that relates rows to each other.  No float anywhere; the same call gives the same bytes.
 * Units.  pairs = 0: a unit is a row, U = n_rows.  pairs = 1: a unit is the pair of rows 2k / 2k + 1, U = n_rows / 2.
 * Key.  With l = rows->d_lens[i] the key of a row is the number k = min(l, key_len) (key_len == 0: k = l) and its base bytes [0, k) as they lie: a byte compare, like
 * the judge's trans.  rows->base_mode is not looked at - lower case differs from upper case, N is a base like any other.  A pair's key is R1's key followed by R2's,
 * both lengths included: (AB, C) and (A, BC) differ, and a pair with its mates swapped differs from the pair.  Bytes at positions >= k - padding, or the tail beyond
 * key_len - never matter; two rows of length 0 are equal.  Lengths cut by rfq_adapter_rows or by the judge come in as rows->d_lens (the composition the judge uses
 * behind the adapter step); a start offset is not offered.  Names are not looked at, quality rows only with RFQ_DEDUP_BEST_QUAL.
 * Candidates.  d_in: [n_rows] bytes, NULL = all.  A unit is a candidate when the byte of every one of its rows is non-zero.  A unit that is no candidate gets keep 0,
 * dup_of -1, count 0 and belongs to no class: a read the judge has failed does not stand in for its passing copies.
 * Classes.  The candidates with identical keys form a class.  Every output is a function of the classes alone - never of a hash, of the table's size or of the order
 * in which the units arrive.  The representative of a class: RFQ_DEDUP_FIRST - its lowest unit index; RFQ_DEDUP_BEST_QUAL - the member with the highest sum of quality
 * bytes over its key window [0, k) (of both mates with pairs), ties to the lowest index.
 * Outputs; each may be NULL and is then not produced, the result is filled either way.  d_keep: [n_rows] bytes, 1 for the rows of a representative, 0 for all others
 * (both rows of a pair get the unit's byte).  d_dup_of: [U] int32, the unit index of the unit's representative (its own for a representative, -1 for a unit that is
 * no candidate).  d_count: [U] uint32, the class size at the representative, 0 elsewhere.  d_hist: [hist_len] uint64, zeroed, then bin c - 1 = the number of classes
 * of size c, the last bin holds every larger class (the convention of rfq_adapter_rows' insert histogram).
 * Result.  n_units = U; n_candidates; n_classes = the kept units; n_dups = n_candidates - n_classes; max_class = the largest class size; bases_in / bases_kept = the
 * sum of l over the rows of the candidates / of the kept units.
 * RFQ_E_ARG, judged on the host: pairs other than 0 / 1, an odd n_rows with pairs; an unknown mode; RFQ_DEDUP_BEST_QUAL without rows->d_quals; row_len == 0, a NULL
 * d_lens or d_bases with rows; row_len above 2^22 (the score is 32 bits); a d_lens / d_dup_of / d_count that is not 4-byte or a d_hist that is not 8-byte aligned;
 * hist_len == 0 with d_hist, or hist_len > 1024; an output that overlaps an input (byte ranges are compared; d_in is an input: the mask is not updated in place);
 * U >= 2^31 - 1.  RFQ_E_ARG, judged on the device, the message names the first such row: lens[i] < 0 or > row_len, of ANY row, candidate or not - what the outputs
 * hold is then unspecified; nothing outside the row buffers is read for such a row.  RFQ_E_HIP when the memory of the table cannot be had; the message says how many
 * bytes.  After any refusal the context stays usable.
 * The table.  Classes are found through a hash table in context-owned device memory: S slots, S the power of two >= max(1024, 2 * U), 20 bytes a slot, and 16 bytes
 * of scratch per unit; it is sized and zeroed PER CALL.  A table carried across the batches of one file - duplicates of a read that came in an earlier call - is
 * not offered: a caller that needs it passes the file's rows in one call.  RFQ_DEDUP=collide keeps four bits of the hash (every probe walks a long chain and every
 * comparison is a byte compare): another formulation of the same result, for the tests.
 * The row buffers may have any alignment, on rfq_judge_rows' terms - whole 16-byte groups with row_len % 16 == 0 and 16-byte alignment, otherwise at their own
 * alignment, never a byte outside [d_x, d_x + n_rows * row_len).  n_rows * row_len may exceed 4 GiB.  Synchronous on the context's stream, one read-back; stage times
 * through rfq_last_timings (dedup:key, dedup:claim, dedup:resolve). */
#define RFQ_DEDUP_FIRST     0
#define RFQ_DEDUP_BEST_QUAL 1
typedef struct {
    int32_t  pairs;                       /* 1: a unit is the pair of rows 2k / 2k + 1 (n_rows must be even)            */
    int32_t  mode;                        /* RFQ_DEDUP_FIRST / RFQ_DEDUP_BEST_QUAL                                      */
    uint32_t key_len;                     /* > 0: only the first key_len bases of a row are its key; 0: the whole read  */
    uint32_t hist_len;                    /* entries of d_hist, <= 1024                                                 */
    const uint8_t* d_in;                  /* [n_rows] bytes, non-zero = the row is a candidate (rfq_judge_rows' d_keep); NULL = every row */
    uint8_t*  d_keep;                     /* [n_rows] 1 / 0, or NULL                                                    */
    int32_t*  d_dup_of;                   /* [U] or NULL                                                                */
    uint32_t* d_count;                    /* [U] or NULL                                                                */
    uint64_t* d_hist;                     /* [hist_len], 8-byte aligned, or NULL                                        */
} rfq_dedup_rows_args;
typedef struct {
    uint64_t n_units, n_candidates, n_classes, n_dups, max_class;
    uint64_t bases_in, bases_kept;
} rfq_dedup_rows_result;
RFQ_API int rfq_dedup_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_dedup_rows_args* args, rfq_dedup_rows_result* res);

/* The QC profile, beside the steps that decide: rows under rfq_select_rows' triple (keep, start, len) -> the tables a QC report is built from (in the manner of fastp's
 * and FastQC's reports; integer rules of this project's own, no parity with either is claimed).  Like rfq_judge_rows it moves no rows: one call on the raw rows is the
 * profile "before filtering", one call with the triple the judge, the adapter step and dedup produce is the profile "after filtering".  No float anywhere, products in
 * 64 bits; the same call gives the same bytes, whatever kernel, grid or order of arrival.  Names and rows->qual_offset are not looked at: a quality byte IS the score.
 * Mates.  M = 1 + pairs.  With pairs row i belongs to mate i & 1 and read 1 and read 2 are profiled apart; without, every row is mate 0.  A row is COUNTED when d_keep
 * is NULL or d_keep[i] != 0 - the pair rule stays the caller's (rfq_dedup_rows and rfq_select_rows write or apply it to both rows of a pair).
 * Window.  [a, a + n) of row i with a = d_start[i] (NULL: 0) and n = d_len[i] (NULL: lens[i] - a).  Position j of the row is cycle c = j - a and is tabulated in table
 * row min(c, cycles - 1): the last row collects what lies beyond (the convention of the family's histograms); the result's max_len, the longest counted window, says
 * whether that happened.
 * Base classes are rfq_adapter_rows': class 0 .. 3 = code 0 .. 3 or A C G T in either case, class 4 (other) = every other byte; GC is class 1 or 2.
 * Outputs, all uint64 and 8-byte aligned; each may be NULL and is then not produced; they are zeroed, then filled, with rows or without.
 *   d_base_cnt   [M][cycles][5]      the counted positions of a cycle and class
 *   d_base_qsum  [M][cycles][5]      the sum of their scores
 *   d_qual_hist  [M][cycles][qbins]  the counted positions of a cycle and score; scores >= qbins - 1 go in the last bin
 *   d_len_hist   [M][len_bins]       the counted rows by min(n, len_bins - 1); a window of 0 is counted in bin 0
 *   d_meanq_hist [M][qbins]          the counted rows with n > 0 by min(qsum / n, qbins - 1), integer division
 *   d_gc_hist    [M][101]            the counted rows with acgt > 0 by 100 * gc / acgt, acgt: the window's positions of class 0 .. 3
 * Quantiles are the caller's, from d_qual_hist; tables of several calls add up (a table carried across calls is not offered).
 * Result, per mate over the windows of the counted rows: counted, bases, qsum, q20, q30 (scores >= 20 / 30), gc, other; max_len; n_rows.  It is filled also when every
 * output is NULL.  The score fields are 0 without rows->d_quals, gc and other without rows->d_bases.
 * RFQ_E_ARG, judged on the host: pairs other than 0 / 1, an odd n_rows with pairs; a bad base_mode; row_len == 0 or a NULL d_lens with rows; cycles outside 1 .. 65536
 * with a per-cycle table; qbins outside 1 .. 256 with a table that has score bins; len_bins == 0 or > 2^20 with d_len_hist; rows->d_quals == NULL with d_base_qsum,
 * d_qual_hist or d_meanq_hist and rows->d_bases == NULL with d_base_cnt, d_base_qsum or d_gc_hist (with rows); a d_lens / d_start / d_len that is not 4-byte or a table
 * that is not 8-byte aligned; an output that overlaps an input or another output (byte ranges are compared); n_rows >= 2^31.  RFQ_E_ARG, judged on the device, the
 * message names the first such row - ALL rows are judged, counted or not: lens[i] < 0 or > row_len; start < 0, len < 0 or start + len > lens[i] (in 64 bits).  What the
 * tables hold is then unspecified; nothing outside the row buffers is read for such a row.  After any refusal the context stays usable.
 * The row buffers may have any alignment, on rfq_judge_rows' terms - never a byte outside [d_x, d_x + n_rows * row_len).  n_rows * row_len may exceed 4 GiB.  Rows of up to
 * 1024 bytes whose tables fit a compute unit's LDS are tabulated there and flushed once per workgroup; longer rows, larger tables (and every call with
 * RFQ_PROFILE=general) add to the tables in device memory position by position - the same bytes, slower.  Synchronous on the context's stream, one read-back; stage time
 * through rfq_last_timings (profile:rows). */
#define RFQ_PROFILE_GC_BINS 101
typedef struct {
    int32_t  pairs;                       /* 1: row i is of mate i & 1 (n_rows must be even)                            */
    uint32_t cycles;                      /* rows of the per-cycle tables, 1 .. 65536                                   */
    uint32_t qbins;                       /* score bins, 1 .. 256                                                       */
    uint32_t len_bins;                    /* entries of d_len_hist per mate, 1 .. 2^20                                  */
    const uint8_t* d_keep;                /* [n_rows] bytes, non-zero = the row is counted; NULL = every row            */
    const int32_t* d_start;               /* [n_rows] or NULL (0)                                                       */
    const int32_t* d_len;                 /* [n_rows] or NULL (to the end of the read)                                  */
    uint64_t* d_base_cnt;                 /* [M][cycles][5] or NULL                                                     */
    uint64_t* d_base_qsum;                /* [M][cycles][5] or NULL                                                     */
    uint64_t* d_qual_hist;                /* [M][cycles][qbins] or NULL                                                 */
    uint64_t* d_len_hist;                 /* [M][len_bins] or NULL                                                      */
    uint64_t* d_meanq_hist;               /* [M][qbins] or NULL                                                         */
    uint64_t* d_gc_hist;                  /* [M][101] or NULL                                                           */
} rfq_profile_rows_args;
typedef struct {
    uint64_t n_rows;
    uint64_t counted[2], bases[2], qsum[2], q20[2], q30[2], gc[2], other[2];   /* [mate]; [1] is 0 without pairs        */
    uint64_t max_len;                     /* the longest counted window                                                 */
} rfq_profile_rows_result;
RFQ_API int rfq_profile_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_profile_rows_args* args, rfq_profile_rows_result* res);

/* Screening against reference k-mers, beside rfq_judge_rows and rfq_dedup_rows: what IS a read - the PhiX spike-in, rRNA, the host, a bait set?  rfq_screen_build
 * makes an exact set of canonical k-mers from reference sequences, rfq_screen_rows counts for every row the k-mers that are in the set and leaves a keep byte (in the
 * manner of BBDuk and FastQ Screen; integer rules of this project's own, no parity with either is claimed).  Like the judge and dedup it DECIDES and moves no bytes:
 * d_keep is what rfq_dedup_rows takes as d_in and rfq_select_rows as d_keep.  No float anywhere; the same call gives the same outputs.
 * Base classes are rfq_adapter_rows': class 0 .. 3 = code 0 .. 3 (RFQ_ROWS_CODE) or A C G T in either case (RFQ_ROWS_ASCII), every other byte is "other".
 * k-mer.  k is 4 .. 31.  The k-mer at position p of a sequence of l bases exists when p + k <= l and is VALID when all its k positions are of class 0 .. 3.  Its forward
 * value is sum class(p + i) * 4^(k - 1 - i), its reverse-complement value sum (3 - class(p + k - 1 - i)) * 4^(k - 1 - i), its canonical value the smaller of the two (a
 * k-mer that is its own reverse complement - even k - is canonical as it stands).
 * rfq_screen_build.  References are ASCII text on the device, a blob and n_refs + 1 uint64 offsets (the layout of rfq_rows_in's names).  The set is every canonical
 * value of every valid k-mer of every reference; k-mers do not span two references.  The index goes into a CALLER-owned device buffer: a 64-byte header (magic,
 * version, k, S, n_kmers, flags) and S 64-bit slots, S the power of two >= max(1024, 2 * refs_len) - known without a read-back; size_only = 1 returns slots and
 * index_bytes and writes nothing.  A slot is 0 (empty) or bit 63 | value; open addressing, a slot is claimed with one compare-and-swap.  WHICH slot a value lands in
 * may depend on the order of arrival: the index BYTES are private and may differ from run to run; the set, n_kmers (the distinct values) and every output of
 * rfq_screen_rows are the same every time.  Result: n_refs, ref_bases (the references' bytes), n_positions (valid k-mers), n_kmers, slots, index_bytes.
 * RFQ_E_ARG, judged on the host: k outside 4 .. 31; a NULL d_refs or d_ref_off with n_refs > 0; a d_ref_off that is not 8-byte or a d_index that is not 16-byte aligned;
 * a NULL d_index on a call that writes; an index that overlaps the references.  RFQ_E_ARG, judged on the device, the message names the first such reference: offsets
 * that decrease or end past refs_len.  RFQ_E_NOSPACE, nothing written, the message says what is needed: index_cap too small.  An empty set (no reference, or none
 * with k valid bases in a row) is NOT an error: every later screen reports 0 hits.
 * rfq_screen_rows.  Units and candidates are rfq_dedup_rows': pairs makes rows 2u / 2u + 1 one unit; d_in NULL = all rows; a unit is a candidate when the byte of every
 * one of its rows is non-zero.  Lengths come from rows->d_lens - what rfq_adapter_rows or the judge cut comes in there; the window is [0, lens[i]).  Names and quality
 * rows are not read.  Outputs; each may be NULL and is then not produced: d_kmers [n_rows] uint32, the row's valid k-mers; d_hits [n_rows] uint32, those whose canonical
 * value is in the set; d_keep [n_rows] bytes.  A row of a unit that is no candidate gets 0 / 0 / 0.  With H and K the unit's sums of hits and k-mers over its rows the
 * unit MATCHES when H >= max(min_hits, 1) and 100 * H >= min_pct * K (64 bits, min_pct 0 .. 100).  RFQ_SCREEN_DROP_MATCHED (contaminant removal): keep = candidate and
 * not matched; RFQ_SCREEN_KEEP_MATCHED (bait): keep = candidate and matched; both rows of a pair get the unit's byte.  Result: n_units, n_candidates, n_matched, n_kept,
 * kmers, hits (sums over the candidates), bases_in / bases_kept (the sum of l over the rows of the candidates / of the kept units).
 * RFQ_E_ARG, judged on the host: pairs other than 0 / 1, an odd n_rows with pairs; an unknown mode; min_pct > 100; a bad base_mode; row_len == 0, a NULL d_lens or
 * d_bases with rows; a NULL or misaligned (16 bytes) d_index, index_bytes < 64; a d_lens / d_kmers / d_hits that is not 4-byte aligned; an output that overlaps an
 * input (byte ranges are compared; the index and d_in are inputs); n_rows >= 2^31.  RFQ_E_DATA for an index whose header is not one rfq_screen_build writes: it is read
 * back once and checked for the magic, the version, k in range, S a power of two and 64 + 8 * S <= index_bytes.  RFQ_E_ARG, judged on the device, the message names
 * the first such row - ALL rows are judged, candidates or not: lens[i] < 0 or > row_len; what the outputs hold is then unspecified.  After any refusal the context
 * stays usable.
 * A probe walk takes at most S steps whatever the slots hold: an index that was written over cannot hang the call.  Nothing outside [d_index, d_index + index_bytes) and
 * the row buffers is read.  The row buffers may have any alignment, on rfq_judge_rows' terms - never a byte outside [d_x, d_x + n_rows * row_len).  n_rows * row_len may
 * exceed 4 GiB.  An index of up to 16384 slots (PhiX, adapter sets, a mitochondrion) is copied into a compute unit's LDS by every workgroup and probed there; a larger
 * one is probed in device memory.  Rows beyond 1024 bytes (and every call with RFQ_SCREEN=general) go to a wave-per-unit kernel with the table in device memory - the
 * same outputs.  RFQ_SCREEN=collide makes rfq_screen_build keep four bits of the hash (recorded in the header's flags, so that every lookup agrees): long probe chains,
 * for the tests.  Synchronous on the context's stream; rfq_screen_rows has one read-back beside the header's; stage times through rfq_last_timings (screen:build,
 * screen:rows).
 * NOT offered: per-reference attribution (build one index per reference and screen once per index, as FastQ Screen does with its genomes); k-mers that tolerate
 * mismatches; k > 31; trimming at a k-mer; a window other than [0, lens[i]). */
#define RFQ_SCREEN_DROP_MATCHED 0
#define RFQ_SCREEN_KEEP_MATCHED 1
typedef struct {
    uint32_t k;                           /* 4 .. 31                                                                    */
    int32_t  size_only;                   /* 1: only slots and index_bytes are reported, nothing is written             */
    const uint8_t*  d_refs; size_t refs_len;            /* the references' ASCII bytes back to back                     */
    const uint64_t* d_ref_off; uint64_t n_refs;         /* [n_refs + 1], 8-byte aligned: reference i is [off[i], off[i + 1]) */
    void* d_index; size_t index_cap;      /* the caller's buffer, 16-byte aligned                                       */
} rfq_screen_build_args;
typedef struct {
    uint64_t n_refs, ref_bases, n_positions, n_kmers, slots, index_bytes;
} rfq_screen_build_result;
RFQ_API int rfq_screen_build(rfq_ctx* ctx, const rfq_screen_build_args* args, rfq_screen_build_result* res);
typedef struct {
    int32_t  pairs;                       /* 1: a unit is the pair of rows 2u / 2u + 1 (n_rows must be even)            */
    int32_t  mode;                        /* RFQ_SCREEN_DROP_MATCHED / RFQ_SCREEN_KEEP_MATCHED                          */
    uint32_t min_hits, min_pct;           /* a unit matches with H >= max(min_hits, 1) and 100 * H >= min_pct * K       */
    const void* d_index; size_t index_bytes;            /* what rfq_screen_build wrote                                  */
    const uint8_t* d_in;                  /* [n_rows] bytes, non-zero = the row is a candidate; NULL = every row        */
    uint32_t* d_kmers;                    /* [n_rows] or NULL                                                           */
    uint32_t* d_hits;                     /* [n_rows] or NULL                                                           */
    uint8_t*  d_keep;                     /* [n_rows] 1 / 0, or NULL                                                    */
} rfq_screen_rows_args;
typedef struct {
    uint64_t n_units, n_candidates, n_matched, n_kept, kmers, hits, bases_in, bases_kept;
} rfq_screen_rows_result;
RFQ_API int rfq_screen_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_screen_rows_args* args, rfq_screen_rows_result* res);

/* Counting canonical k-mers, beside rfq_screen_rows: WHICH k-mers do the reads hold, and how often - the k-mer section of a QC report, the k-mer spectrum (genome
 * size, error rate, the valley between error k-mers and real ones), screening by abundance.  rfq_kmers_init formats a table in a CALLER-owned device buffer,
 * rfq_kmers_rows adds the k-mers of rows to it, rfq_kmers_read takes out its spectrum, its (value, count) list and a screen index of selected values.  The table is the
 * caller's and survives between calls: several rfq_kmers_rows calls on one table give the table of the concatenated rows, in whatever order the calls came - the
 * one result of the rows family that adds up across the batches of a file.  No float anywhere; the same calls give the same outputs.
 * The k-mer rules are rfq_screen_*'s, word for word: k is 4 .. 31; base classes are rfq_adapter_rows'; a k-mer is VALID when all its k positions are of class 0 .. 3;
 * its canonical value is the smaller of its forward and reverse-complement values; a k-mer that is its own reverse complement counts once per occurrence.
 * The table, 16-byte aligned: a 64-byte header (a magic of its own, version, k, S, n_kmers, total, flags), S slots of 64 bits - 0 = empty, else bit 63 | canonical
 * value: the screen index's slot format and linear probing, its hash taken of the value mixed once more (the k-mers of reads share suffixes - poly-A and poly-G
 * tails, repeats - as reference k-mers do not) - and S counts of 64 bits, count[s] beside slot[s].  WHICH slot a value lands in may differ from run
 * to run: the table BYTES are private; the set of (value, count) pairs, the header's counts and every output of the calls below are the same every time.
 * rfq_kmers_init.  slots is what the caller asks for; S is the power of two >= max(1024, slots), table_bytes = 64 + 16 * S.  SIZING RULE: slots >= 2 x the distinct
 * values expected (at most 4^k / 2 + 2^k / 2 values exist at all: 512 for k = 5).  size_only = 1 reports slots (S) and table_bytes and writes nothing; otherwise the
 * header is written and the rest zeroed.  RFQ_E_ARG: k outside 4 .. 31, slots > 2^36, a misaligned d_table, a NULL d_table on a call that writes, more than 65536 slots
 * under RFQ_KMERS=collide.  RFQ_E_NOSPACE, nothing written, the message says what is needed: table_cap too small.  RFQ_KMERS=collide at the time of the call is
 * recorded in the header's flags: later calls agree with it whatever the switch says then.
 * rfq_kmers_rows adds 1 to count[value] for every valid k-mer of every COUNTED row.  A row is counted when d_in is NULL or d_in[i] != 0 (rfq_profile_rows' rule: no
 * pairs here, the pair rule is already in the mask).  The window is [0, rows->d_lens[i]) - what rfq_adapter_rows or the judge cut comes in there.  Names and quality
 * rows are not read.  d_kmers [n_rows] uint32, optional: the row's valid k-mers, 0 for a row that is not counted - for the same rows and mask rfq_screen_rows' d_kmers
 * byte for byte.  Result: n_rows, n_counted, bases_in (the sum of l over the counted rows), added (the occurrences this call added), n_new (the values this call
 * claimed), n_kmers and total (the table's distinct values and sum of counts after the call, also written to the header), lost.
 * A table that is too full: a probe walk takes at most min(S, W) steps, W = 512 (S under the recorded collide flag).  A k-mer whose walk ends without an empty slot
 * or its own value is LOST.  With lost > 0 the call returns RFQ_E_NOSPACE (the message gives lost, n_kmers and S; the result fields stay filled in) and the header
 * gets an INCOMPLETE flag: every later rfq_kmers_rows or rfq_kmers_read on that table is RFQ_E_DATA until rfq_kmers_init formats it again.  A call is therefore
 * either exact or refused, never silently short; with slots >= 2 x the distinct values no walk comes near W.
 * RFQ_E_ARG, judged on the host: a bad base_mode; row_len == 0, a NULL d_lens or d_bases with rows; a NULL or misaligned (16 bytes) d_table, table_bytes < 64; a
 * d_lens / d_kmers that is not 4-byte aligned; d_kmers overlapping an input (the table and d_in are inputs) or the table overlapping an input; n_rows >= 2^31.
 * RFQ_E_DATA, after one read-back of the header: a magic or version that is not rfq_kmers_init's (a screen index handed in as a table is refused that way; a table
 * handed to rfq_screen_rows is refused by that call's magic check), k out of range, S no power of two or 64 + 16 * S > table_bytes, the INCOMPLETE flag.  RFQ_E_ARG,
 * judged on the device, the message names the first such row - ALL rows are judged, counted or not: lens[i] < 0 or > row_len; the table then holds the k-mers of the
 * other counted rows (such a row adds none) and its header says so.  After any refusal the context stays usable.
 * Every slot number is masked to S and every walk bounded: a table whose bytes were written over cannot hang a call or make it read or write outside
 * [d_table, d_table + table_bytes).  ONE table takes ONE call at a time: two contexts (or two streams) counting into one table at once is NOT offered.
 * rfq_kmers_read.  An entry is SELECTED when max(min_count, 1) <= count and (max_count == 0 or count <= max_count).  Outputs; each may be NULL and is then not
 * produced: d_hist [hist_len] uint64, hist_len <= 65536 - zeroed first; bin c - 1 = the number of distinct values with count c over ALL entries, the last bin collects
 * every larger count (the family's convention): the k-mer spectrum; d_values / d_counts [list_cap] uint64 each - the selected entries, the value without bit 63 and
 * its count, at the same position of both; their order is unspecified, the set is the same every time; d_index / index_cap - a screen index of the selected values,
 * S_idx the power of two >= max(1024, 2 * n_selected), the header what rfq_screen_build writes (its flags by RFQ_SCREEN at the time of the call), n_kmers =
 * n_selected: rfq_screen_rows takes it unchanged - the bridge to screening by abundance.  size_only = 1 fills the result and writes nothing.  Result: k, slots,
 * n_kmers, total, max_count (the largest count in the table), n_selected, selected_total, index_slots, index_bytes.  An empty table reads as empty, its index is the
 * empty set.  RFQ_E_NOSPACE, nothing written, the message says what is needed: list_cap < n_selected with a list, index_cap < index_bytes with d_index.  RFQ_E_ARG:
 * the table arguments as above; hist_len > 65536 or 0 with d_hist; d_hist / d_values / d_counts not 8-byte, d_index not 16-byte aligned; an output that overlaps the
 * table or another output.  RFQ_E_DATA: the header checks of rfq_kmers_rows; slots that do not hold what the header counts.
 * Rows of up to 1024 bytes are held whole; a workgroup combines its k-mers in a table in LDS and flushes it once (a hot value - poly-A, an adapter, every value at k =
 * 5 - costs one 64-bit atomic per workgroup, not one per occurrence).  RFQ_KMERS=direct leaves the LDS stage out, RFQ_KMERS=general takes the wave-per-row kernel
 * for every row length; every value gives the same table contents and outputs.  Synchronous on the context's stream; stage times through rfq_last_timings
 * (kmers:init, kmers:rows, kmers:read).
 * NOT offered: per-cycle k-mer tables; k > 31; counts per reference; a top-N on the device (sort d_counts); two writers on one table. */
typedef struct {
    uint32_t k;                           /* 4 .. 31                                                                    */
    int32_t  size_only;                   /* 1: only slots and table_bytes are reported, nothing is written             */
    uint64_t slots;                       /* asked for: >= 2 x the distinct values expected                             */
    void* d_table; size_t table_cap;      /* the caller's buffer, 16-byte aligned                                       */
} rfq_kmers_init_args;
typedef struct {
    uint64_t slots, table_bytes;
} rfq_kmers_init_result;
RFQ_API int rfq_kmers_init(rfq_ctx* ctx, const rfq_kmers_init_args* args, rfq_kmers_init_result* res);
typedef struct {
    void* d_table; size_t table_bytes;    /* what rfq_kmers_init formatted                                              */
    const uint8_t* d_in;                  /* [n_rows] bytes, non-zero = the row is counted; NULL = every row            */
    uint32_t* d_kmers;                    /* [n_rows] or NULL                                                           */
} rfq_kmers_rows_args;
typedef struct {
    uint64_t n_rows, n_counted, bases_in, added, n_new, n_kmers, total, lost;
} rfq_kmers_rows_result;
RFQ_API int rfq_kmers_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_kmers_rows_args* args, rfq_kmers_rows_result* res);
typedef struct {
    const void* d_table; size_t table_bytes;
    uint64_t min_count, max_count;        /* selected: max(min_count, 1) <= count and (max_count == 0 or count <= max_count) */
    int32_t  size_only;                   /* 1: the result is filled, nothing is written                                */
    uint32_t hist_len;                    /* bins of d_hist, <= 65536                                                   */
    uint64_t* d_hist;                     /* [hist_len] or NULL                                                         */
    uint64_t* d_values; uint64_t* d_counts; size_t list_cap;      /* [list_cap] each, or NULL                           */
    void* d_index; size_t index_cap;      /* a screen index of the selected values, 16-byte aligned, or NULL            */
} rfq_kmers_read_args;
typedef struct {
    uint64_t k, slots, n_kmers, total, max_count, n_selected, selected_total, index_slots, index_bytes;
} rfq_kmers_read_result;
RFQ_API int rfq_kmers_read(rfq_ctx* ctx, const rfq_kmers_read_args* args, rfq_kmers_read_result* res);

/* Demultiplexing, in front of every other step of the rows family: WHOSE read is this?  A pooled run carries the sample in an inline barcode at the front of R1,
 * sometimes a second one at the front of R2; index reads handed over as rows of their own do the same job.  rfq_demux_rows compares a fixed window of every row with
 * a set of barcodes and leaves, per unit, the sample - and the keep byte and the start rfq_select_rows takes, so that one rfq_select_rows call per sample splits the
 * batch and cuts the barcode off (integer rules of this project's own, in the manner of cutadapt's demultiplexing, fastq-multx and bcl2fastq's --barcode-mismatches;
 * no parity with any of them is claimed).  Like the judge it DECIDES and moves no bytes.  No float anywhere; the same call gives the same bytes.
 * Units and candidates are rfq_dedup_rows': pairs = 0, a unit is a row; pairs = 1, a unit is rows 2u / 2u + 1; d_in NULL = every row; a unit is a candidate when the
 * byte of every one of its rows is non-zero.  U is the number of units.
 * Barcode sets.  Set 1 is n1 barcodes of len1 bases each, HOST bytes h_bc1[n1][len1], A C G T in either case; it is read from the row at [off1, off1 + len1) of row u
 * (row 2u with pairs).  The optional set 2 (n2, len2, off2, h_bc2) is for pairs only and is read from row 2u + 1.  1 <= len <= 32, 1 <= n <= 4096 per set, with set 2
 * n1 * n2 <= 2^20.  Two equal barcodes in one set are refused.
 * Distance.  Base classes are rfq_adapter_rows': class 0 .. 3 = code 0 .. 3 (RFQ_ROWS_CODE) or A C G T in either case (RFQ_ROWS_ASCII), every other byte is "other".  A
 * position AGREES when the row's byte is of class 0 .. 3 and equals the barcode's class; a byte of class other (N) never agrees.  dist(row, b) is the number of the len
 * positions that do not agree.  A row with lens[i] < off + len has no window: it sets RFQ_DEMUX_SHORT and nothing of it is compared.
 * Match of a row within its set.  best is the lowest index among the barcodes at the least distance d1; d2 is the least distance among all OTHER barcodes (len + 1
 * when the set has one barcode).  The row MATCHES when d1 <= max_mm and d2 - d1 >= min_delta: min_delta = 0 lets the lowest index win a tie, 1 asks for a unique
 * best.  Otherwise it sets RFQ_DEMUX_NONE (d1 > max_mm) or RFQ_DEMUX_AMBIG.  max_mm <= 32, min_delta <= 33.
 * Sample of a unit.  One set: the sample is best, n_samples = n1.  Two sets, h_pairs NULL: sample = best1 * n2 + best2, n_samples = n1 * n2.  Two sets with a sample
 * sheet h_pairs[n_samples][2], HOST int32 pairs (i, j): sample s is the pair listed s-th, 1 <= n_samples <= 65536, every index in range and no pair listed twice; a
 * unit whose two rows both match but whose pair is not listed sets RFQ_DEMUX_COMBO - the index-hopping count of a dual-indexed run.  why is the OR of the bits of
 * the unit's rows; the unit is ASSIGNED when it is a candidate and why == 0.
 * Outputs; each may be NULL and is then not produced, the result is filled either way.  d_sample [U] int32: the sample, or -1.  d_why [U] uint8: the RFQ_DEMUX_*
 * bits; a unit that is no candidate gets RFQ_DEMUX_MASKED alone.  d_best [n_rows] int32: the row's best - set for every candidate row that has a window, matched or
 * not; -1 for a row without a set, without a window, or of a unit that is no candidate.  d_dist [n_rows] uint8: d1 wherever d_best is set, 255 wherever it is -1.
 * d_keep [n_rows] uint8: 1 for the rows of an assigned unit, 0 otherwise.  d_start [n_rows] int32, what rfq_select_rows takes as d_start: for a row of an ASSIGNED
 * unit that has a set min(lens[i], off + len + skip) - skip1 / skip2 are linker bases cut with the barcode, the prefix [0, off) goes too -, 0 for every other row: the
 * unassigned bin keeps its reads whole.  d_counts [n_samples + 1] uint64, 8-byte aligned, zeroed then filled: the candidate units per sample, the last entry the
 * candidate units that were not assigned.  Result: n_units, n_candidates, n_assigned, n_samples; n_exact, the assigned units whose every compared distance is 0;
 * why_none, why_ambig, why_short, why_combo, the units with that bit; bases_in, the sum of l over the rows of the candidates; bases_out, the sum of l - start over the
 * rows of the assigned units.
 * RFQ_E_ARG, judged on the host: pairs other than 0 / 1, an odd n_rows with pairs; set 2, h_pairs, skip2 or off2 without pairs, h_pairs without set 2; no set 1; a
 * length, count, max_mm or min_delta out of range; a barcode byte other than ACGTacgt, duplicate barcodes, a bad sample sheet; off + len + skip not representable in
 * int32; a bad base_mode; row_len == 0, a NULL d_lens or d_bases with rows; a d_lens / d_sample / d_best / d_start that is not 4-byte or a d_counts that is not 8-byte
 * aligned; an output that overlaps an input or another output (byte ranges are compared; d_in is an input); n_rows >= 2^31.  RFQ_E_ARG, judged on the device, the
 * message names the first such row - ALL rows are judged, candidates or not: lens[i] < 0 or > row_len; what the outputs hold is then unspecified, and nothing outside
 * the row buffers is read.  After any refusal the context stays usable.
 * The row buffers may have any alignment, on rfq_judge_rows' terms - never a byte outside [d_bases, d_bases + n_rows * row_len).  n_rows * row_len may exceed 4 GiB.
 * Quality rows and names are not read.  The host packs every barcode into 2-bit classes and uploads the sets - and the dense [n1][n2] table it makes of the sample
 * sheet - per call into scratch of the context's that only grows.  One kernel: a lane per unit, the sets in a compute unit's LDS (at most 34 KiB), the counts in an LDS table of up
 * to 8192 cells flushed once per workgroup (beyond that 64-bit atomic adds in device memory).  RFQ_DEMUX=general takes the other formulation - a lane per unit
 * compares byte by byte against the barcodes' ASCII bytes in device memory - with the same bytes in every output.  Synchronous on the context's stream, one read-back;
 * stage time through rfq_last_timings (demux:rows).
 * NOT offered: barcodes of different lengths within one set, indels, a barcode searched at several offsets or at the 3' end, N as a wildcard in a barcode; barcodes
 * read out of the name line.  UMI extraction is rfq_select_rows' tag (rfq_name_tag: the bases behind the barcode go into the kept names; d_start here says where
 * they begin).  Grouping the rows by sample in one pass is rfq_group_rows' (d_bin = d_sample). */
#define RFQ_DEMUX_NONE   1                /* d1 > max_mm                                                                */
#define RFQ_DEMUX_AMBIG  2                /* d2 - d1 < min_delta                                                        */
#define RFQ_DEMUX_SHORT  4                /* lens[i] < off + len: no window                                             */
#define RFQ_DEMUX_COMBO  8                /* both rows matched, the pair is not in the sample sheet                     */
#define RFQ_DEMUX_MASKED 128              /* the unit is no candidate                                                   */
typedef struct {
    int32_t  pairs;                       /* 1: a unit is the pair of rows 2u / 2u + 1 (n_rows must be even)            */
    uint32_t n1, len1, off1, skip1;       /* set 1: barcodes, bases each, the window's start, linker bases behind it    */
    const uint8_t* h_bc1;                 /* HOST [n1][len1] ACGTacgt                                                   */
    uint32_t n2, len2, off2, skip2;       /* set 2 (pairs only, read from row 2u + 1); n2 == 0 and h_bc2 NULL: none     */
    const uint8_t* h_bc2;                 /* HOST [n2][len2] or NULL                                                    */
    const int32_t* h_pairs;               /* HOST [n_samples][2] (i, j), or NULL: every combination, i * n2 + j         */
    uint32_t n_samples;                   /* rows of h_pairs, 1 .. 65536; ignored without h_pairs                       */
    uint32_t max_mm, min_delta;           /* a row matches with d1 <= max_mm and d2 - d1 >= min_delta                   */
    const uint8_t* d_in;                  /* [n_rows] bytes, non-zero = the row is a candidate; NULL = every row        */
    int32_t*  d_sample;                   /* [U] or NULL                                                                */
    uint8_t*  d_why;                      /* [U] or NULL                                                                */
    int32_t*  d_best;                     /* [n_rows] or NULL                                                           */
    uint8_t*  d_dist;                     /* [n_rows] or NULL                                                           */
    uint8_t*  d_keep;                     /* [n_rows] 1 / 0, or NULL                                                    */
    int32_t*  d_start;                    /* [n_rows] or NULL                                                           */
    uint64_t* d_counts;                   /* [n_samples + 1], 8-byte aligned, or NULL                                   */
} rfq_demux_rows_args;
typedef struct {
    uint64_t n_units, n_candidates, n_assigned, n_samples, n_exact, why_none, why_ambig, why_short, why_combo, bases_in, bases_out;
} rfq_demux_rows_result;
RFQ_API int rfq_demux_rows(rfq_ctx* ctx, const rfq_rows_in* rows, const rfq_demux_rows_args* args, rfq_demux_rows_result* res);

/* stage timings of the last batch / rows call, in milliseconds, measured with HIP events on the context's stream.
 * names[i] is a static string; returns the number of stages written (<= cap). */
RFQ_API int rfq_last_timings(const rfq_ctx* ctx, const char** names, float* ms, int cap);

/* device-memory helpers for hosts that do not bring their own allocator (the C++ driver, ctypes tests): thin wrappers
 * over hipMalloc / hipFree / hipMemcpy on the context's device.  Buffers from rfq_dev_malloc are 256-byte aligned. */
RFQ_API int rfq_dev_malloc(rfq_ctx* ctx, void** d_ptr, size_t n);
RFQ_API int rfq_dev_free(rfq_ctx* ctx, void* d_ptr);
RFQ_API int rfq_copy_h2d(rfq_ctx* ctx, void* d_dst, const void* h_src, size_t n);
/* The same without waiting: the copy is queued on the context's copy stream (h_src page-locked: rfq_host_alloc) and runs beside whatever the
 * context's own stream does.  *ticket (optional) identifies it: rfq_copy_done says whether it has finished (the host buffer may be reused),
 * rfq_copy_sync waits for everything queued so far - call it before handing the destination to rfq_encode_batch / rfq_decode_batch. */
RFQ_API int rfq_copy_h2d_async(rfq_ctx* ctx, void* d_dst, const void* h_src, size_t n, uint64_t* ticket);
RFQ_API int rfq_copy_done(rfq_ctx* ctx, uint64_t ticket);      /* 1: finished, 0: still running, < 0: error */
RFQ_API int rfq_copy_sync(rfq_ctx* ctx);
RFQ_API int rfq_copy_d2h(rfq_ctx* ctx, void* h_dst, const void* d_src, size_t n);
RFQ_API int rfq_copy_d2d(rfq_ctx* ctx, void* d_dst, const void* d_src, size_t n);
/* d_dst on ctx's GPU <- d_src on src_ctx's GPU (hipMemcpyPeerAsync): how a worker of a multi-GPU host queue pulls its byte range */
RFQ_API int rfq_copy_peer(rfq_ctx* ctx, void* d_dst, const rfq_ctx* src_ctx, const void* d_src, size_t n);
/* page-locked host buffers (hipHostMalloc): H2D / D2H copies from them run at full PCIe rate */
RFQ_API int rfq_host_alloc(rfq_ctx* ctx, void** h_ptr, size_t n);
RFQ_API int rfq_host_free(rfq_ctx* ctx, void* h_ptr);
/* the same for memory the caller owns (hipHostRegister / hipHostUnregister): buffers a host filled before the context existed */
RFQ_API int rfq_host_register(rfq_ctx* ctx, void* h_ptr, size_t n);
RFQ_API int rfq_host_unregister(rfq_ctx* ctx, void* h_ptr);

/* --compare on the device (Repaq::compare / comparePE, src/repaq.cpp:36-233): the first offset at which two device texts differ,
 * *first_diff = n when they are identical.  A decoded batch equal byte for byte to the same span of the FASTQ text passes the
 * reference's four per-read tests (name, sequence, strand, quality; :85-108) for every read in it; the host cuts records only in
 * a batch that differs, to word the reference's message. */
RFQ_API int rfq_compare_bytes(rfq_ctx* ctx, const void* d_a, const void* d_b, size_t n, uint64_t* first_diff);

/* Test / diagnostic switches of one context: name = the RFQ_* environment variable of the same meaning (RFQ_GATHER=old, RFQ_QUAL=bytes|masks, RFQ_CODER=list|mask, RFQ_INDEX=2pass,
 * RFQ_IDX_TILES, RFQ_STREAMS=1, RFQ_SLICE_BYTES, RFQ_SLICE_BASES, RFQ_WALK=exact, RFQ_GW_SHIFT, RFQ_MATERIALISE=1, RFQ_TRACE, RFQ_G2_PAD, RFQ_SP_PAD, RFQ_JUDGE=general, RFQ_ADAPTER=general, RFQ_MERGE=general, RFQ_DEDUP=collide, RFQ_PROFILE=general, RFQ_SCREEN=general|collide, RFQ_KMERS=general|collide|direct, RFQ_DEMUX=general, RFQ_TAG=general; see RfqOpts in
 * repaq_amd/csrc/rfq_ctx.h), value NULL or "" = default.  Every switch selects another formulation of the same, bit-identical result - they exist so that
 * the tests can pin each one (tests/test_gpu_formulations.py forces every one of them on the GPU).  Unknown names and values that are not of the switch's
 * form or range are RFQ_E_ARG.  The environment is read once, by rfq_create; the batch calls never call getenv. */
RFQ_API int rfq_set_option(rfq_ctx* ctx, const char* name, const char* value);
/* the switch's current value in the form rfq_set_option takes ("" = default), so that a caller can put back what it found */
RFQ_API int rfq_get_option(const rfq_ctx* ctx, const char* name, char* out, size_t cap);
/* the switches' names: i = 0, 1, ... until NULL */
RFQ_API const char* rfq_option_name(int i);

/* self test of the wave-level scans / reductions every kernel is built on (DPP row shifts and broadcasts on gfx950): h_in holds 64 * n_waves lane
 * values, h_out receives 12 u64 per lane (see k_selftest_wave in rfq_api.hip); tests/test_wave_primitives.py checks them against a serial reference. */
RFQ_API int rfq_selftest_wave(rfq_ctx* ctx, const uint64_t* h_in, uint32_t n_waves, uint64_t* h_out);

/* library / build info: "rfq_hip <version> gfx950" (or "... simt-emulation" for the test build) */
RFQ_API const char* rfq_version(void);

#ifdef __cplusplus
}
#endif
#endif
