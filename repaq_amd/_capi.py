"""ctypes binding of the C-ABI in include/rfq_hip.h (librfq_hip.so, built by hipcc for gfx950).

There is no CPU implementation behind this module: if the shared library is missing or no GPU is usable, loading /
Engine() raises.  (tests/ may point RFQ_HIP_LIBRARY at tests/emu/librfq_emu.so, the SIMT-interpreter TEST build of the
same sources, to debug kernel logic on a GPU-less box; nothing in repaq_amd does that on its own.)"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "lib", "librfq_hip.so")

RFQ_OK = 0
SE, PE_TWO_FILES, PE_INTERLEAVED = 0, 1, 2
HEADER_MAX = 17 + 255
U64_MAX = (1 << 64) - 1
ERRORS = {-1: "RFQ_E_NO_DEVICE", -2: "RFQ_E_HIP", -3: "RFQ_E_ARG", -4: "RFQ_E_TEXT", -5: "RFQ_E_DATA", -6: "RFQ_E_FORMAT",
          -7: "RFQ_E_UNPINNED", -8: "RFQ_E_NOSPACE", -9: "RFQ_E_STATE"}


class RfqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERRORS.get(code, code), msg))
        self.code = code
        self.message = msg


class EncodeArgs(C.Structure):
    _fields_ = [("d_fq1", C.c_void_p), ("n1", C.c_size_t), ("d_fq2", C.c_void_p), ("n2", C.c_size_t), ("paired", C.c_int32),
                ("chunk_bases", C.c_uint32), ("final", C.c_int32), ("emit_header", C.c_int32), ("file_off1", C.c_uint64),
                ("file_off2", C.c_uint64), ("nolb_from1", C.c_uint64), ("nolb_from2", C.c_uint64), ("d_out", C.c_void_p), ("out_cap", C.c_size_t),
                ("flush_all", C.c_int32), ("carry_bases", C.c_uint32)]


class EncodeResult(C.Structure):
    _fields_ = [("d_rfq", C.c_void_p), ("rfq_len", C.c_size_t), ("n_chunks", C.c_uint32), ("n_reads", C.c_uint64), ("n_bases", C.c_uint64),
                ("consumed1", C.c_size_t), ("consumed2", C.c_size_t), ("h_chunk_off", C.POINTER(C.c_uint64)),
                ("input_ended", C.c_int32), ("reserved", C.c_int32)]


class ScanResult(C.Structure):
    _fields_ = [("n_chunks", C.c_uint32), ("n_reads", C.c_uint64), ("consumed1", C.c_size_t), ("consumed2", C.c_size_t),
                ("h_end1", C.POINTER(C.c_uint64)), ("h_end2", C.POINTER(C.c_uint64)), ("input_ended", C.c_int32), ("unit_bases", C.c_uint32)]


class DecodeArgs(C.Structure):
    _fields_ = [("d_rfq", C.c_void_p), ("n", C.c_size_t), ("has_header", C.c_int32), ("split_pe", C.c_int32), ("final", C.c_int32), ("bug_compat", C.c_int32),
                ("d_out1", C.c_void_p), ("cap1", C.c_size_t), ("d_out2", C.c_void_p), ("cap2", C.c_size_t),
                ("h_chunk_off", C.POINTER(C.c_uint64)), ("n_chunk_off", C.c_uint32), ("reserved3", C.c_uint32)]


class DecodeResult(C.Structure):
    _fields_ = [("d_fq1", C.c_void_p), ("n1", C.c_size_t), ("d_fq2", C.c_void_p), ("n2", C.c_size_t), ("n_chunks", C.c_uint32),
                ("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("consumed", C.c_size_t)]


ROWS_ASCII, ROWS_CODE = 0, 1


class DecodeRowsArgs(C.Structure):
    _fields_ = [("d_rfq", C.c_void_p), ("n", C.c_size_t), ("has_header", C.c_int32), ("final", C.c_int32),
                ("h_chunk_off", C.POINTER(C.c_uint64)), ("n_chunk_off", C.c_uint32), ("row_len", C.c_uint32), ("base_mode", C.c_int32),
                ("qual_offset", C.c_uint8), ("pad_base", C.c_uint8), ("pad_qual", C.c_uint8), ("reserved", C.c_uint8),
                ("d_bases", C.c_void_p), ("bases_cap", C.c_size_t), ("d_quals", C.c_void_p), ("quals_cap", C.c_size_t),
                ("d_lens", C.c_void_p), ("lens_cap", C.c_size_t)]


class DecodeRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("n_chunks", C.c_uint32), ("max_len", C.c_uint32), ("consumed", C.c_size_t)]


class DecodeNamesArgs(C.Structure):
    _fields_ = [("d_rfq", C.c_void_p), ("n", C.c_size_t), ("has_header", C.c_int32), ("final", C.c_int32),
                ("h_chunk_off", C.POINTER(C.c_uint64)), ("n_chunk_off", C.c_uint32), ("size_only", C.c_int32),
                ("d_names", C.c_void_p), ("names_cap", C.c_size_t), ("d_name_off", C.c_void_p), ("off_cap", C.c_size_t)]


class DecodeNamesResult(C.Structure):
    _fields_ = [("d_names", C.c_void_p), ("names_len", C.c_uint64), ("d_name_off", C.c_void_p), ("n_rows", C.c_uint64), ("n_chunks", C.c_uint32),
                ("max_name", C.c_uint32), ("consumed", C.c_size_t)]


class RowsIn(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("row_len", C.c_uint32), ("base_mode", C.c_int32), ("qual_offset", C.c_uint8), ("reserved", C.c_uint8 * 3),
                ("d_bases", C.c_void_p), ("d_quals", C.c_void_p), ("d_lens", C.c_void_p), ("d_names", C.c_void_p), ("names_len", C.c_size_t),
                ("d_name_off", C.c_void_p)]


class RowsTextResult(C.Structure):
    _fields_ = [("d_fq1", C.c_void_p), ("n1", C.c_size_t), ("d_fq2", C.c_void_p), ("n2", C.c_size_t), ("n_reads", C.c_uint64), ("n_bases", C.c_uint64)]


class TextRowsArgs(C.Structure):
    _fields_ = [("d_fq1", C.c_void_p), ("n1", C.c_size_t), ("d_fq2", C.c_void_p), ("n2", C.c_size_t), ("paired", C.c_int32), ("final", C.c_int32),
                ("file_off1", C.c_uint64), ("file_off2", C.c_uint64), ("row_len", C.c_uint32), ("base_mode", C.c_int32),
                ("qual_offset", C.c_uint8), ("pad_base", C.c_uint8), ("pad_qual", C.c_uint8), ("reserved", C.c_uint8),
                ("d_bases", C.c_void_p), ("bases_cap", C.c_size_t), ("d_quals", C.c_void_p), ("quals_cap", C.c_size_t),
                ("d_lens", C.c_void_p), ("lens_cap", C.c_size_t), ("d_names", C.c_void_p), ("names_cap", C.c_size_t),
                ("d_name_off", C.c_void_p), ("off_cap", C.c_size_t)]


class TextRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("names_len", C.c_uint64), ("max_len", C.c_uint32), ("max_name", C.c_uint32),
                ("consumed1", C.c_size_t), ("consumed2", C.c_size_t), ("input_ended", C.c_int32), ("reserved", C.c_int32)]


TAG_PART_MAX, TAG_PREFIX_MAX, TAG_AT_SPACE, TAG_AT_END = 32, 14, 0, 1


class NameTag(C.Structure):
    _fields_ = [("d_tag_start", C.c_void_p), ("d_tag_len", C.c_void_p), ("h_prefix", C.c_char_p), ("prefix_len", C.c_uint32),
                ("sep", C.c_uint8), ("join", C.c_uint8), ("at", C.c_uint8), ("reserved", C.c_uint8)]


class SelectRowsArgs(C.Structure):
    _fields_ = [("d_keep", C.c_void_p), ("d_start", C.c_void_p), ("d_len", C.c_void_p), ("pairs", C.c_int32), ("min_len", C.c_uint32), ("row_len", C.c_uint32),
                ("pad_base", C.c_uint8), ("pad_qual", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("d_bases", C.c_void_p), ("bases_cap", C.c_size_t), ("d_quals", C.c_void_p), ("quals_cap", C.c_size_t),
                ("d_lens", C.c_void_p), ("lens_cap", C.c_size_t), ("d_names", C.c_void_p), ("names_cap", C.c_size_t),
                ("d_name_off", C.c_void_p), ("off_cap", C.c_size_t), ("tag", C.POINTER(NameTag))]


class SelectRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("names_len", C.c_uint64), ("max_len", C.c_uint32), ("max_name", C.c_uint32),
                ("n_in", C.c_uint64), ("dropped_mask", C.c_uint64), ("dropped_short", C.c_uint64), ("dropped_mate", C.c_uint64)]


class GroupRowsArgs(C.Structure):
    _fields_ = [("d_keep", C.c_void_p), ("d_start", C.c_void_p), ("d_len", C.c_void_p), ("pairs", C.c_int32), ("min_len", C.c_uint32),
                ("d_bin", C.c_void_p), ("n_bins", C.c_uint32), ("rest", C.c_int32), ("d_bin_off", C.c_void_p), ("bin_cap", C.c_size_t), ("row_len", C.c_uint32),
                ("pad_base", C.c_uint8), ("pad_qual", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("d_bases", C.c_void_p), ("bases_cap", C.c_size_t), ("d_quals", C.c_void_p), ("quals_cap", C.c_size_t),
                ("d_lens", C.c_void_p), ("lens_cap", C.c_size_t), ("d_names", C.c_void_p), ("names_cap", C.c_size_t),
                ("d_name_off", C.c_void_p), ("off_cap", C.c_size_t)]


class GroupRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("names_len", C.c_uint64), ("max_len", C.c_uint32), ("max_name", C.c_uint32),
                ("n_in", C.c_uint64), ("dropped_mask", C.c_uint64), ("dropped_short", C.c_uint64), ("dropped_mate", C.c_uint64), ("dropped_bin", C.c_uint64),
                ("n_bins_used", C.c_uint32), ("reserved", C.c_uint32)]


CUT_FRONT, CUT_RIGHT, CUT_TAIL = 1, 2, 4
WHY_SHORT, WHY_N, WHY_MEANQ, WHY_LOWQ, WHY_COMPLEX = 1, 2, 4, 8, 16


class JudgeRowsArgs(C.Structure):
    _fields_ = [("trim_front", C.c_uint32), ("trim_tail", C.c_uint32), ("poly_g", C.c_uint32), ("cut_flags", C.c_uint32), ("cut_window", C.c_uint32),
                ("cut_mean_q", C.c_uint32), ("max_len", C.c_uint32), ("min_len", C.c_uint32), ("max_n", C.c_int32), ("min_mean_q", C.c_uint32),
                ("qual_q", C.c_uint32), ("max_lowq_pct", C.c_uint32), ("min_complexity_pct", C.c_uint32), ("reserved", C.c_uint32),
                ("d_keep", C.c_void_p), ("d_start", C.c_void_p), ("d_len", C.c_void_p), ("d_why", C.c_void_p), ("d_metrics", C.c_void_p)]


class JudgeRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_rows", "n_kept", "why_short", "why_n", "why_meanq", "why_lowq", "why_complex", "bases_in", "qsum_in", "q20_in",
                                          "q30_in", "bases_out", "qsum_out", "q20_out", "q30_out")]


CUT_BY_OVERLAP, CUT_BY_ADAPTER = 1, 2


class AdapterRowsArgs(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("min_overlap", C.c_uint32), ("max_diff", C.c_uint32), ("max_diff_pct", C.c_uint32),
                ("h_adapter1", C.c_char_p), ("adapter1_len", C.c_uint32), ("h_adapter2", C.c_char_p), ("adapter2_len", C.c_uint32),
                ("adapter_min", C.c_uint32), ("adapter_mm_per", C.c_uint32), ("hist_len", C.c_uint32),
                ("d_len", C.c_void_p), ("d_how", C.c_void_p), ("d_insert", C.c_void_p), ("d_diff", C.c_void_p), ("d_insert_hist", C.c_void_p)]


class AdapterRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_rows", "n_pairs", "pairs_found", "rows_cut", "rows_cut_overlap", "rows_cut_adapter", "bases_in", "bases_out")]


class MergeRowsArgs(C.Structure):
    _fields_ = [("d_insert", C.c_void_p), ("row_len", C.c_uint32), ("pad_base", C.c_uint8), ("pad_qual", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("d_bases", C.c_void_p), ("bases_cap", C.c_size_t), ("d_quals", C.c_void_p), ("quals_cap", C.c_size_t),
                ("d_lens", C.c_void_p), ("lens_cap", C.c_size_t), ("d_names", C.c_void_p), ("names_cap", C.c_size_t),
                ("d_name_off", C.c_void_p), ("off_cap", C.c_size_t)]


class MergeRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_bases", C.c_uint64), ("names_len", C.c_uint64), ("max_len", C.c_uint32), ("max_name", C.c_uint32),
                ("n_pairs", C.c_uint64), ("overlap_bases", C.c_uint64)]


DEDUP_FIRST, DEDUP_BEST_QUAL = 0, 1


class DedupRowsArgs(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("mode", C.c_int32), ("key_len", C.c_uint32), ("hist_len", C.c_uint32), ("d_in", C.c_void_p),
                ("d_keep", C.c_void_p), ("d_dup_of", C.c_void_p), ("d_count", C.c_void_p), ("d_hist", C.c_void_p)]


class DedupRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_units", "n_candidates", "n_classes", "n_dups", "max_class", "bases_in", "bases_kept")]


PROFILE_GC_BINS = 101
PROFILE_TABLES = ("base_cnt", "base_qsum", "qual_hist", "len_hist", "meanq_hist", "gc_hist")


class ProfileRowsArgs(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("cycles", C.c_uint32), ("qbins", C.c_uint32), ("len_bins", C.c_uint32), ("d_keep", C.c_void_p), ("d_start", C.c_void_p),
                ("d_len", C.c_void_p)] + [("d_" + t, C.c_void_p) for t in PROFILE_TABLES]


class ProfileRowsResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64)] + [(f, C.c_uint64 * 2) for f in ("counted", "bases", "qsum", "q20", "q30", "gc", "other")] + [("max_len", C.c_uint64)]


SCREEN_DROP_MATCHED, SCREEN_KEEP_MATCHED = 0, 1
SCREEN_HEADER_BYTES = 64


class ScreenBuildArgs(C.Structure):
    _fields_ = [("k", C.c_uint32), ("size_only", C.c_int32), ("d_refs", C.c_void_p), ("refs_len", C.c_size_t), ("d_ref_off", C.c_void_p), ("n_refs", C.c_uint64),
                ("d_index", C.c_void_p), ("index_cap", C.c_size_t)]


class ScreenBuildResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_refs", "ref_bases", "n_positions", "n_kmers", "slots", "index_bytes")]


class ScreenRowsArgs(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("mode", C.c_int32), ("min_hits", C.c_uint32), ("min_pct", C.c_uint32), ("d_index", C.c_void_p), ("index_bytes", C.c_size_t),
                ("d_in", C.c_void_p), ("d_kmers", C.c_void_p), ("d_hits", C.c_void_p), ("d_keep", C.c_void_p)]


class ScreenRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_units", "n_candidates", "n_matched", "n_kept", "kmers", "hits", "bases_in", "bases_kept")]


KMERS_HEADER_BYTES = 64


class KmersInitArgs(C.Structure):
    _fields_ = [("k", C.c_uint32), ("size_only", C.c_int32), ("slots", C.c_uint64), ("d_table", C.c_void_p), ("table_cap", C.c_size_t)]


class KmersInitResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("slots", "table_bytes")]


class KmersRowsArgs(C.Structure):
    _fields_ = [("d_table", C.c_void_p), ("table_bytes", C.c_size_t), ("d_in", C.c_void_p), ("d_kmers", C.c_void_p)]


class KmersRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_rows", "n_counted", "bases_in", "added", "n_new", "n_kmers", "total", "lost")]


class KmersReadArgs(C.Structure):
    _fields_ = [("d_table", C.c_void_p), ("table_bytes", C.c_size_t), ("min_count", C.c_uint64), ("max_count", C.c_uint64), ("size_only", C.c_int32),
                ("hist_len", C.c_uint32), ("d_hist", C.c_void_p), ("d_values", C.c_void_p), ("d_counts", C.c_void_p), ("list_cap", C.c_size_t),
                ("d_index", C.c_void_p), ("index_cap", C.c_size_t)]


class KmersReadResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("k", "slots", "n_kmers", "total", "max_count", "n_selected", "selected_total", "index_slots", "index_bytes")]


DEMUX_NONE, DEMUX_AMBIG, DEMUX_SHORT, DEMUX_COMBO, DEMUX_MASKED = 1, 2, 4, 8, 128


class DemuxRowsArgs(C.Structure):
    _fields_ = [("pairs", C.c_int32), ("n1", C.c_uint32), ("len1", C.c_uint32), ("off1", C.c_uint32), ("skip1", C.c_uint32), ("h_bc1", C.c_char_p),
                ("n2", C.c_uint32), ("len2", C.c_uint32), ("off2", C.c_uint32), ("skip2", C.c_uint32), ("h_bc2", C.c_char_p),
                ("h_pairs", C.POINTER(C.c_int32)), ("n_samples", C.c_uint32), ("max_mm", C.c_uint32), ("min_delta", C.c_uint32), ("d_in", C.c_void_p),
                ("d_sample", C.c_void_p), ("d_why", C.c_void_p), ("d_best", C.c_void_p), ("d_dist", C.c_void_p), ("d_keep", C.c_void_p), ("d_start", C.c_void_p),
                ("d_counts", C.c_void_p)]


class DemuxRowsResult(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_units", "n_candidates", "n_assigned", "n_samples", "n_exact", "why_none", "why_ambig", "why_short", "why_combo",
                                          "bases_in", "bases_out")]


_libs = {}


def load(path=None):
    path = path or os.environ.get("RFQ_HIP_LIBRARY") or DEFAULT_LIB
    if path in _libs:
        return _libs[path]
    try:
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HSA runtimes in one process cannot both
        # open the GPU, so when torch is around let it load its runtime first; librfq_hip.so then binds to the same one
        # (same SONAME).  Hosts without torch (the C++ driver) simply use /opt/rocm's.
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(path):
        raise ImportError("librfq_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); repaq_amd has no CPU fallback" % path)
    L = C.CDLL(path)
    L.rfq_version.restype = C.c_char_p
    L.rfq_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.rfq_destroy.argtypes = [C.c_void_p]
    L.rfq_last_error.argtypes = [C.c_void_p]; L.rfq_last_error.restype = C.c_char_p
    L.rfq_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.rfq_set_header.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rfq_get_header.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t)]
    L.rfq_clear_header.argtypes = [C.c_void_p]; L.rfq_clear_header.restype = None
    L.rfq_encode_batch.argtypes = [C.c_void_p, C.POINTER(EncodeArgs), C.POINTER(EncodeResult)]
    L.rfq_decode_batch.argtypes = [C.c_void_p, C.POINTER(DecodeArgs), C.POINTER(DecodeResult)]
    L.rfq_decode_rows.argtypes = [C.c_void_p, C.POINTER(DecodeRowsArgs), C.POINTER(DecodeRowsResult)]
    L.rfq_decode_names.argtypes = [C.c_void_p, C.POINTER(DecodeNamesArgs), C.POINTER(DecodeNamesResult)]
    L.rfq_rows_to_text.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(RowsTextResult)]
    L.rfq_encode_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(EncodeArgs), C.POINTER(EncodeResult)]
    L.rfq_text_rows.argtypes = [C.c_void_p, C.POINTER(TextRowsArgs), C.POINTER(TextRowsResult)]
    L.rfq_select_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(SelectRowsArgs), C.POINTER(SelectRowsResult)]
    L.rfq_group_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(GroupRowsArgs), C.POINTER(GroupRowsResult)]
    L.rfq_judge_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(JudgeRowsArgs), C.POINTER(JudgeRowsResult)]
    L.rfq_adapter_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(AdapterRowsArgs), C.POINTER(AdapterRowsResult)]
    L.rfq_merge_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(MergeRowsArgs), C.POINTER(MergeRowsResult)]
    L.rfq_dedup_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(DedupRowsArgs), C.POINTER(DedupRowsResult)]
    L.rfq_profile_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(ProfileRowsArgs), C.POINTER(ProfileRowsResult)]
    L.rfq_screen_build.argtypes = [C.c_void_p, C.POINTER(ScreenBuildArgs), C.POINTER(ScreenBuildResult)]
    L.rfq_screen_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(ScreenRowsArgs), C.POINTER(ScreenRowsResult)]
    L.rfq_kmers_init.argtypes = [C.c_void_p, C.POINTER(KmersInitArgs), C.POINTER(KmersInitResult)]
    L.rfq_kmers_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(KmersRowsArgs), C.POINTER(KmersRowsResult)]
    L.rfq_kmers_read.argtypes = [C.c_void_p, C.POINTER(KmersReadArgs), C.POINTER(KmersReadResult)]
    L.rfq_demux_rows.argtypes = [C.c_void_p, C.POINTER(RowsIn), C.POINTER(DemuxRowsArgs), C.POINTER(DemuxRowsResult)]
    L.rfq_scan_batch.argtypes = [C.c_void_p, C.POINTER(EncodeArgs), C.POINTER(ScanResult)]
    L.rfq_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    L.rfq_dev_malloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    L.rfq_dev_free.argtypes = [C.c_void_p, C.c_void_p]
    L.rfq_copy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.rfq_copy_h2d_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.rfq_copy_done.argtypes = [C.c_void_p, C.c_uint64]
    L.rfq_copy_sync.argtypes = [C.c_void_p]
    L.rfq_copy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rfq_copy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rfq_copy_peer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.rfq_host_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    L.rfq_host_free.argtypes = [C.c_void_p, C.c_void_p]
    L.rfq_compare_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    L.rfq_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.rfq_get_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.rfq_option_name.argtypes = [C.c_int]; L.rfq_option_name.restype = C.c_char_p
    L.rfq_selftest_wave.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64)]
    _libs[path] = L
    return L


EXPORTS = ["rfq_version", "rfq_create", "rfq_destroy", "rfq_last_error", "rfq_set_stream", "rfq_set_header", "rfq_get_header", "rfq_clear_header",
           "rfq_encode_batch", "rfq_scan_batch", "rfq_decode_batch", "rfq_decode_rows", "rfq_decode_names", "rfq_rows_to_text", "rfq_encode_rows", "rfq_text_rows", "rfq_select_rows", "rfq_group_rows", "rfq_judge_rows", "rfq_adapter_rows", "rfq_merge_rows", "rfq_dedup_rows", "rfq_profile_rows", "rfq_screen_build", "rfq_screen_rows", "rfq_kmers_init", "rfq_kmers_rows", "rfq_kmers_read", "rfq_demux_rows", "rfq_last_timings", "rfq_dev_malloc", "rfq_dev_free", "rfq_copy_h2d", "rfq_copy_d2h",
           "rfq_copy_h2d_async", "rfq_copy_done", "rfq_copy_sync",
           "rfq_copy_d2d", "rfq_copy_peer", "rfq_host_alloc", "rfq_host_free", "rfq_compare_bytes", "rfq_selftest_wave", "rfq_set_option", "rfq_get_option", "rfq_option_name", "rfq_host_register", "rfq_host_unregister"]
