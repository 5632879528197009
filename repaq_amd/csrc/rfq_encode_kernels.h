// rfq_encode_kernels.h — gfx950 kernels of the FASTQ -> RFQ encode path (included by rfq_encode.hip only).
//
// Pipeline (one batch = whole FASTQ stream(s) resident in HBM; reference call sites in brackets):
//   index    k_nl_bitmap -> scan -> k_line_offsets            newline bitmap, global line ranks, line-start table
//            [FastqReader::getLine/read, src/fastqreader.cpp:94-196, for '\n'-terminated text]
//   table    k_read_table                                     per-read lengths + FastqMeta::parse [src/fastqmeta.cpp:22-80]
//   cut      scan + k_partition                               chunk boundaries [Repaq::compress, src/repaq.cpp:546-553]
//   header   k_hdr_*                                          RfqCodec::makeHeader + makeQualityTable on chunk 0
//   chunk    k_chunk_flags, k_overlap, scans, k_gather, k_stream_plan, k_pos_coder, k_coords, k_chunk_layout,
//            k_assemble*                                      RfqCodec::encodeChunk + RfqChunk::write
#pragma once
// The kernels live in enc/*.h by stage (one 244 KB header was unreviewable); this file is the order they are included in.
#include "enc/tables.h"                       // the batch's text, per-read and per-chunk tables
#include "enc/index.h"                        // line index (one pass with a decoupled look-back; two-pass fallback) and the text normaliser of the slow path
#include "enc/reads_cut.h"                    // name parse, read lengths, chunk partition
#include "enc/hdr_from_chunk0.h"              // the file header from chunk 0 (makeHeader, makeQualityTable)
#include "enc/chunk_flags_overlap.h"          // per-chunk flag words, interleave test, the overlap search, stored prefixes
#include "enc/gather_bytes.h"                 // byte-wise gather (reads that do not fit a tile) + the counters both gathers share
#include "enc/gather_tiles.h"                 // tile gather k_gather2 (names parsed, match masks, bases packed where they stand), sequence packer, stream plan
#include "enc/pos_coder.h"                    // position coder: a wave per (chunk, value streams, segment)
#include "enc/pos_coder_list.h"               // position coder for many value streams: work follows the coded positions
#include "enc/coords.h"                       // coordinate coder (encodeCoords)
#include "enc/assemble.h"                     // chunk layout (incl. the mSize bug) and image assembly
#include "enc/rows_text.h"                    // rows -> FASTQ text in front of the encoder (rfq_rows_to_text, rfq_encode_rows)
#include "enc/text_rows.h"                    // FASTQ text -> rows, lengths and names from the line index (rfq_text_rows)
#include "enc/rows_lanes.h"                   // what the rows kernels below share: group reductions, 16-byte pieces, the deciding calls' walk, length check, candidate test and sums
#include "enc/rows_select.h"                  // rows -> the kept rows, trimmed, with their names (rfq_select_rows)
#include "enc/rows_tag.h"                     // a tag of the read's own bases written into the kept names of rfq_select_rows: the judge's rule, the plan, the two names writers (rfq_name_tag)
#include "enc/rows_group.h"                   // rows -> the kept rows grouped by a bin per unit in one pass, trimmed, with their names and the first row of every bin (rfq_group_rows)
#include "enc/rows_judge.h"                   // rows -> keep, window, reason and metrics per row + a QC summary (rfq_judge_rows)
#include "enc/rows_adapter.h"                 // rows -> the length adapter removal leaves, insert sizes of the pairs + a summary (rfq_adapter_rows)
#include "enc/rows_merge.h"                   // pairs -> one read per overlapping pair, the consensus of both mates, with R1's names (rfq_merge_rows)
#include "enc/rows_kmer_lanes.h"              // what the kernels below that read bases 2 bits at a time share: a lane's 16 positions, the k-mers of a row, the set of slots and its one claim (behind rows_adapter.h for ar_bits / ar_cls)
#include "enc/rows_dedup.h"                   // rows -> a keep byte that leaves one unit of every class of identical units, class sizes + a summary (rfq_dedup_rows)
#include "enc/rows_profile.h"                 // rows under a keep / start / length triple -> per-cycle base content, position x score, length / mean-quality / GC tables (rfq_profile_rows)
#include "enc/rows_screen.h"                  // references -> an index of canonical k-mers; rows against it -> k-mers, hits and a keep byte per row + a summary (rfq_screen_build, rfq_screen_rows)
#include "enc/rows_kmers.h"                   // rows -> a caller-owned table of canonical k-mers with counts that adds up across calls; the table -> spectrum, (value, count) list, a screen index (rfq_kmers_init, rfq_kmers_rows, rfq_kmers_read)
#include "enc/rows_demux.h"                   // rows against one or two sets of barcodes -> a sample per unit, the keep byte and start rfq_select_rows takes, counts per sample + a summary (rfq_demux_rows)
