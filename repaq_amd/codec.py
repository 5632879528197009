"""Host-side mirror of the reference's RfqCodec seam (src/rfqcodec.h:17-43) over the C-ABI.

    reference                                   here
    RfqCodec codec;                             codec = RfqCodec(device=0)
    codec.setHeader(h)                          codec.setHeader(header_bytes)
    h = codec.makeHeader(reads)  (chunk 0)      implicit in the first encode (header from the first chunk), codec.header()
    chunk = codec.encodeChunk(reads); write     codec.encode(d_fq1, n1, ...) -> EncodeResult (all chunks of the batch)
    reads = codec.decodeChunk(chunk)            codec.decode(d_rfq, n, ...)  -> DecodeResult (FASTQ text of all chunks)

Pointers are device pointers (e.g. torch.uint8 CUDA tensors' data_ptr()).  The *_bytes helpers move host bytes through
rfq_dev_malloc / rfq_copy_* for tests and small tools."""
import ctypes as C

from . import _capi as A
from ._capi import RfqError, SE, PE_TWO_FILES, PE_INTERLEAVED, U64_MAX  # noqa: F401


def _chunk_index(chunk_off, n_chunks):
    """a caller's chunk index - a POINTER(c_uint64) with n_chunks, or a sequence of n_chunks + 1 offsets - as the (h_chunk_off, n_chunk_off) of an args struct"""
    if chunk_off is None:
        return None, 0
    if not isinstance(chunk_off, C.POINTER(C.c_uint64)):
        n_chunks = len(chunk_off) - 1
        chunk_off = C.cast((C.c_uint64 * len(chunk_off))(*chunk_off), C.POINTER(C.c_uint64))
    return (chunk_off if n_chunks else None), n_chunks


class RfqCodec:
    def __init__(self, device=0, library=None):
        self._L = A.load(library)
        h = C.c_void_p()
        rc = self._L.rfq_create(C.byref(h), device)
        if rc != A.RFQ_OK:
            raise RfqError(rc, "rfq_create(device=%d) failed: no usable MI355X / HIP device (there is no CPU fallback)" % device)
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.rfq_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != A.RFQ_OK:
            raise RfqError(rc, self._L.rfq_last_error(self._h).decode("latin-1"))

    def _call(self, fn, Result, *structs, more=()):
        """THE call step: the entry point `fn` on this context with the argument structs by reference, `more` as it stands and a new Result behind them; a status
        other than RFQ_OK raises RfqError with the context's message -> the result struct"""
        r = Result()
        self._check(getattr(self._L, fn)(self._h, *map(C.byref, structs), *more, C.byref(r)))
        return r

    @staticmethod
    def _raw(a, raw):
        """raw: fields of an argument struct set as given (the tests' refusals)"""
        for k, v in (raw or {}).items():
            setattr(a, k, v)

    def version(self):
        return self._L.rfq_version().decode()

    def set_stream(self, stream_ptr):
        self._check(self._L.rfq_set_stream(self._h, stream_ptr))

    def set_option(self, name, value=None):
        """rfq_set_option: a test / diagnostic switch of this context (names = the RFQ_* environment variables; None = default)."""
        self._check(self._L.rfq_set_option(self._h, name.encode(), None if value is None else str(value).encode()))

    def get_option(self, name) -> str:
        """rfq_get_option: the switch's current value ("" = default)"""
        buf = C.create_string_buffer(64)
        self._check(self._L.rfq_get_option(self._h, name.encode(), buf, 64))
        return buf.value.decode()

    def option_names(self):
        """rfq_option_name: every switch the library knows"""
        out, i = [], 0
        while True:
            n = self._L.rfq_option_name(i)
            if not n:
                return out
            out.append(n.decode()); i += 1

    def option(self, name, value):
        """with codec.option("RFQ_GATHER", "old"): ... - the switch set for the block, back to what it WAS afterwards (an environment-provided
        or earlier value, not necessarily the built-in default)"""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self.get_option(name)
            self.set_option(name, value)
            try:
                yield self
            finally:
                self.set_option(name, before or None)
        return scope()

    def selftest_wave(self, lanes):
        """rfq_selftest_wave: the wave scans / reductions of rfq_common.h on `lanes` (64 * k u64 values) -> 12 u64 per lane."""
        n = len(lanes); assert n and n % 64 == 0
        a = (C.c_uint64 * n)(*lanes); o = (C.c_uint64 * (12 * n))()
        self._check(self._L.rfq_selftest_wave(self._h, a, n // 64, o))
        return [list(o[12 * i: 12 * i + 12]) for i in range(n)]

    # --- RfqCodec::setHeader / header accessors
    def setHeader(self, header_bytes: bytes):
        self._check(self._L.rfq_set_header(self._h, header_bytes, len(header_bytes)))

    def clearHeader(self):
        self._L.rfq_clear_header(self._h)

    def header(self) -> bytes:
        buf = C.create_string_buffer(A.HEADER_MAX); n = C.c_size_t()
        self._check(self._L.rfq_get_header(self._h, buf, C.byref(n)))
        return buf.raw[: n.value]

    # --- RfqCodec::encodeChunk for every chunk of a batch
    def encode(self, d_fq1, n1, d_fq2=None, n2=0, paired=SE, chunk_bases=1_000_000, final=True, emit_header=True,
               file_off1=0, file_off2=0, nolb_from1=U64_MAX, nolb_from2=U64_MAX, d_out=None, out_cap=0, flush_all=False):
        a = A.EncodeArgs(d_fq1, n1, d_fq2, n2, paired, chunk_bases, 1 if final else 0, 1 if emit_header else 0,
                         file_off1, file_off2, nolb_from1, nolb_from2, d_out, out_cap, 1 if flush_all else 0, 0)
        return self._call("rfq_encode_batch", A.EncodeResult, a)

    # --- the plan pass of a chunk-parallel encode: where every chunk ends in the input stream(s)
    def scan(self, d_fq1, n1, d_fq2=None, n2=0, paired=SE, chunk_bases=1_000_000, final=True, file_off1=0, file_off2=0, carry_bases=0):
        """rfq_scan_batch: the plan pass.  carry_bases: bases the chunk that is open at the start of this text took from the text in front of it."""
        a = A.EncodeArgs(d_fq1, n1, d_fq2, n2, paired, chunk_bases, 1 if final else 0, 0, file_off1, file_off2, U64_MAX, U64_MAX, None, 0, 0, carry_bases)
        r = self._call("rfq_scan_batch", A.ScanResult, a)
        ends1 = [r.h_end1[i] for i in range(r.n_chunks)]
        ends2 = [r.h_end2[i] for i in range(r.n_chunks)] if (paired == PE_TWO_FILES and r.n_chunks) else []
        return r, ends1, ends2

    # --- RfqCodec::decodeChunk for every chunk of an image
    def decode(self, d_rfq, n, has_header=True, split_pe=False, final=True, d_out1=None, cap1=0, d_out2=None, cap2=0, chunk_off=None, n_chunks=0, bug_compat=False):
        """chunk_off / n_chunks: optional chunk index (EncodeResult.h_chunk_off + n_chunks, or a sequence of n_chunks + 1 offsets).
        bug_compat: with split_pe, lose what Repaq::decompressPE loses behind a non-last NO_LINE_BREAK chunk (src/repaq.cpp:376-403); Repaq::decompress (one output) loses nothing."""
        chunk_off, n_chunks = _chunk_index(chunk_off, n_chunks)
        a = A.DecodeArgs(d_rfq, n, 1 if has_header else 0, 1 if split_pe else 0, 1 if final else 0, 1 if bug_compat else 0, d_out1, cap1, d_out2, cap2,
                         chunk_off, n_chunks, 0)
        return self._call("rfq_decode_batch", A.DecodeResult, a)

    # --- the reads of an image as fixed-stride rows (rfq_decode_rows)
    def decode_rows(self, d_rfq, n, row_len=0, codes=False, qual_offset=33, pad_base=255, pad_qual=255, d_bases=None, bases_cap=0, d_quals=None, quals_cap=0,
                    d_lens=None, lens_cap=0, has_header=True, final=True, chunk_off=None, n_chunks=0):
        """rfq_decode_rows: row i of d_bases / d_quals (device buffers of n_rows * row_len bytes) = read i of decode(split_pe=False), padded to row_len;
        d_lens: n_rows int32 read lengths.  No output buffer given (row_len=0 and no pointers) = a size query: n_rows, n_chunks, max_len, consumed.
        codes: bases as A0 C1 G2 T3 N4; quality bytes are the characters minus qual_offset.  Returns DecodeRowsResult."""
        chunk_off, n_chunks = _chunk_index(chunk_off, n_chunks)
        a = A.DecodeRowsArgs(d_rfq, n, 1 if has_header else 0, 1 if final else 0, chunk_off,
                             n_chunks, row_len, A.ROWS_CODE if codes else A.ROWS_ASCII, qual_offset, pad_base, pad_qual, 0,
                             d_bases, bases_cap, d_quals, quals_cap, d_lens, lens_cap)
        return self._call("rfq_decode_rows", A.DecodeRowsResult, a)

    def decode_rows_bytes(self, rfq: bytes, row_len=None, codes=False, qual_offset=33, pad_base=255, pad_qual=255, bases=True, quals=True, lens=True, **kw):
        """host bytes in, numpy arrays out: (n_rows, max_len, bases [n, L] uint8, quals [n, L] uint8, lens [n] int32) - None for an output not asked
        for.  row_len=None: the image's longest read (a size query first)."""
        import numpy as np
        d = self.dev_put(rfq); bufs = []
        try:
            q = self.decode_rows(d, len(rfq), **kw)
            L = max(q.max_len, 1) if row_len is None else int(row_len)
            n = q.n_rows; nb = max(n * L, 1)
            ob = self.dev_put(b"\0" * nb) if bases else None
            oq = self.dev_put(b"\0" * nb) if quals else None
            ol = self.dev_put(b"\0" * max(4 * n, 4)) if lens else None
            bufs = [x for x in (ob, oq, ol) if x is not None]
            r = self.decode_rows(d, len(rfq), row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad_base, pad_qual=pad_qual,
                                 d_bases=ob, bases_cap=n * L, d_quals=oq, quals_cap=n * L, d_lens=ol, lens_cap=n, **kw)
            n = r.n_rows

            def rows(p):
                return np.frombuffer(self.dev_get(p, n * L), dtype=np.uint8).reshape(n, L) if p is not None else None
            lv = np.frombuffer(self.dev_get(ol, 4 * n), dtype=np.int32) if ol is not None else None
            return n, r.max_len, rows(ob), rows(oq), lv
        finally:
            self.dev_free(d)
            for p in bufs:
                self.dev_free(p)

    # --- the name lines of the same rows (rfq_decode_names)
    def decode_names(self, d_rfq, n, size_only=False, d_names=None, names_cap=0, d_name_off=None, off_cap=0, has_header=True, final=True, chunk_off=None, n_chunks=0):
        """rfq_decode_names: name i = the first line of read i of decode(split_pe=False), '@' included, no line break - all of them back to back at
        d_names and n_rows + 1 uint64 offsets at d_name_off, the layout rows_to_text / encode_rows take.  Row i is row i of decode_rows.  No buffers given =
        context-owned results, valid until the next call; size_only: the counts alone.  The text of the strand lines is not carried (rows always write
        "+").  Returns DecodeNamesResult (d_names, names_len, d_name_off, n_rows, n_chunks, max_name, consumed)."""
        chunk_off, n_chunks = _chunk_index(chunk_off, n_chunks)
        a = A.DecodeNamesArgs(d_rfq, n, 1 if has_header else 0, 1 if final else 0, chunk_off,
                              n_chunks, 1 if size_only else 0, d_names, names_cap, d_name_off, off_cap)
        return self._call("rfq_decode_names", A.DecodeNamesResult, a)

    def decode_names_bytes(self, rfq: bytes, **kw):
        """host bytes in, the list of name lines (bytes, '@' included) out"""
        import numpy as np
        d = self.dev_put(rfq)
        try:
            r = self.decode_names(d, len(rfq), **kw)
            n = int(r.n_rows)
            off = np.frombuffer(self.dev_get(r.d_name_off, 8 * (n + 1)), dtype=np.uint64)
            blob = self.dev_get(r.d_names, int(r.names_len)) if r.names_len else b""
            return [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
        finally:
            self.dev_free(d)

    # --- the way back: fixed-stride rows -> FASTQ text (rfq_rows_to_text) -> image (rfq_encode_rows)
    @staticmethod
    def _rows_in(n_rows, row_len, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, codes, qual_offset, base_mode=None):
        """base_mode: the C constant as it stands instead of `codes`, for callers that keep the C constants (and the tests of the refusal)"""
        mode = base_mode if base_mode is not None else (A.ROWS_CODE if codes else A.ROWS_ASCII)
        return A.RowsIn(n_rows, row_len, mode, qual_offset, (C.c_uint8 * 3)(), d_bases, d_quals, d_lens, d_names, names_len, d_name_off)

    def rows_to_text(self, n_rows, row_len, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, paired=SE, codes=False, qual_offset=33,
                     d_out1=None, cap1=0, d_out2=None, cap2=0, size_only=False):
        """rfq_rows_to_text: rows in the layout of decode_rows (device pointers; d_lens int32, d_name_off n_rows + 1 uint64 offsets into the name lines
        d_names) -> the FASTQ text(s).  No output buffer = context-owned texts, valid until the next call.  Returns RowsTextResult."""
        a = self._rows_in(n_rows, row_len, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, codes, qual_offset)
        return self._call("rfq_rows_to_text", A.RowsTextResult, a, more=(paired, d_out1, cap1, d_out2, cap2, 1 if size_only else 0))

    def encode_rows(self, n_rows, row_len, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, paired=SE, codes=False, qual_offset=33,
                    chunk_bases=1_000_000, final=True, emit_header=True, file_off1=0, file_off2=0, nolb_from1=U64_MAX, nolb_from2=U64_MAX,
                    d_out=None, out_cap=0, flush_all=False, d_fq1=None):
        """rfq_encode_rows: rows_to_text into the context's own text, then encode() on it (final or flush_all: a rows batch is encoded whole).
        d_fq1 exists for the tests of the refusal: the call fills the text in itself.  Returns EncodeResult."""
        a = self._rows_in(n_rows, row_len, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, codes, qual_offset)
        e = A.EncodeArgs(d_fq1, 0, None, 0, paired, chunk_bases, 1 if final else 0, 1 if emit_header else 0,
                         file_off1, file_off2, nolb_from1, nolb_from2, d_out, out_cap, 1 if flush_all else 0, 0)
        return self._call("rfq_encode_rows", A.EncodeResult, a, e)

    def _put_rows(self, bases, quals, lens, names):
        """numpy rows + a list of name lines -> device buffers: (pointers to free, positional arguments of rows_to_text / encode_rows)"""
        import numpy as np
        bases = np.ascontiguousarray(bases, dtype=np.uint8); quals = np.ascontiguousarray(quals, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = int(lens.shape[0]); L = int(bases.shape[1]) if bases.ndim == 2 else 0
        assert bases.shape == quals.shape == (n, L) and len(names) == n and L >= 1, "bases / quals [n, L], lens [n], n names"
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum(np.fromiter((len(x) for x in names), dtype=np.uint64, count=n))
        blob = b"".join(names)
        ptrs = [self.dev_put(x) for x in (bases.tobytes(), quals.tobytes(), lens.tobytes(), blob, off.tobytes())]
        return ptrs, (n, L, ptrs[0], ptrs[1], ptrs[2], ptrs[3], len(blob), ptrs[4])

    def rows_to_text_bytes(self, bases, quals, lens, names, paired=SE, codes=False, qual_offset=33):
        """host convenience: numpy bases / quals [n, L] uint8, lens [n], a list of n name lines (bytes, '@' included) -> the text, or the pair of
        texts with PE_TWO_FILES"""
        ptrs, rows = self._put_rows(bases, quals, lens, names)
        try:
            r = self.rows_to_text(*rows, paired=paired, codes=codes, qual_offset=qual_offset)
            a = self.dev_get(r.d_fq1, r.n1) if r.n1 else b""
            b = self.dev_get(r.d_fq2, r.n2) if (paired == PE_TWO_FILES and r.n2) else b""
            return (a, b) if paired == PE_TWO_FILES else a
        finally:
            for p in ptrs:
                self.dev_free(p)

    def encode_rows_bytes(self, bases, quals, lens, names, paired=SE, chunk_bases=1_000_000, codes=False, qual_offset=33, **kw) -> bytes:
        """host convenience: the same inputs -> the .rfq image (kw: the flags of encode())"""
        ptrs, rows = self._put_rows(bases, quals, lens, names)
        try:
            r = self.encode_rows(*rows, paired=paired, codes=codes, qual_offset=qual_offset, chunk_bases=chunk_bases, **kw)
            return self.dev_get(r.d_rfq, r.rfq_len) if r.rfq_len else b""
        finally:
            for p in ptrs:
                self.dev_free(p)

    # --- the front door: FASTQ text -> rows, lengths and names (rfq_text_rows)
    def text_rows(self, d_fq1, n1, d_fq2=None, n2=0, paired=SE, final=True, file_off1=0, file_off2=0, row_len=0, codes=False, qual_offset=33,
                  pad_base=255, pad_qual=255, d_bases=None, bases_cap=0, d_quals=None, quals_cap=0, d_lens=None, lens_cap=0,
                  d_names=None, names_cap=0, d_name_off=None, off_cap=0):
        """rfq_text_rows: row i of d_bases / d_quals (n_rows * row_len bytes each) = record i the reference's reader makes of the text(s) - the
        records encode() would encode -, d_lens n_rows int32 lengths, d_names / d_name_off the name lines and their n_rows + 1 uint64 offsets (the
        layout rows_to_text / encode_rows take).  No output pointer at all = a size query; an output that is None is not produced.  The bytes are
        the text's own (nothing is lost that an image would lose); codes: A0 C1 G2 T3 N4, any other base is refused.  Returns TextRowsResult
        (n_rows, n_bases, names_len, max_len, max_name, consumed1, consumed2, input_ended)."""
        a = A.TextRowsArgs(d_fq1, n1, d_fq2, n2, paired, 1 if final else 0, file_off1, file_off2, row_len, A.ROWS_CODE if codes else A.ROWS_ASCII,
                           qual_offset, pad_base, pad_qual, 0, d_bases, bases_cap, d_quals, quals_cap, d_lens, lens_cap, d_names, names_cap, d_name_off, off_cap)
        return self._call("rfq_text_rows", A.TextRowsResult, a)

    def text_rows_bytes(self, fq1: bytes, fq2: bytes = b"", paired=SE, row_len=None, codes=False, qual_offset=33, pad_base=255, pad_qual=255, final=True, **kw):
        """host bytes in, numpy arrays out: (result of the call, bases [n, L] uint8, quals [n, L] uint8, lens [n] int32, the list of name lines).
        row_len=None: the text's longest read (a size query first)."""
        import numpy as np
        two = paired == PE_TWO_FILES
        d1 = self.dev_put(fq1); d2 = self.dev_put(fq2) if two else None
        bufs = [d1] + ([d2] if two else [])
        try:
            src = dict(d_fq2=d2, n2=len(fq2) if two else 0, paired=paired, final=final, **kw)
            q = self.text_rows(d1, len(fq1), **src)
            n = int(q.n_rows); L = max(int(q.max_len), 1) if row_len is None else int(row_len); nl = int(q.names_len)
            ob, oq, ol, on, oo = (self.dev_put(b"\0" * max(k, 1)) for k in (n * L, n * L, 4 * n, nl, 8 * (n + 1)))
            bufs += [ob, oq, ol, on, oo]
            r = self.text_rows(d1, len(fq1), row_len=L, codes=codes, qual_offset=qual_offset, pad_base=pad_base, pad_qual=pad_qual,
                               d_bases=ob, bases_cap=n * L, d_quals=oq, quals_cap=n * L, d_lens=ol, lens_cap=n, d_names=on, names_cap=nl,
                               d_name_off=oo, off_cap=n + 1, **src)
            n = int(r.n_rows)
            B = np.frombuffer(self.dev_get(ob, n * L), dtype=np.uint8).reshape(n, L)
            Q = np.frombuffer(self.dev_get(oq, n * L), dtype=np.uint8).reshape(n, L)
            lens = np.frombuffer(self.dev_get(ol, 4 * n), dtype=np.int32)
            off = np.frombuffer(self.dev_get(oo, 8 * (n + 1)), dtype=np.uint64)
            blob = self.dev_get(on, int(r.names_len)) if r.names_len else b""
            return r, B, Q, lens, [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
        finally:
            for p in bufs:
                self.dev_free(p)

    # --- the step in the middle: rows -> the kept rows, trimmed, with their names (rfq_select_rows)
    def select_rows(self, n_rows, row_len_in, d_bases, d_quals, d_lens, d_names=None, names_len=0, d_name_off=None, d_keep=None, d_start=None, d_len=None,
                    pairs=False, min_len=1, row_len=0, pad_base=255, pad_qual=255, out_bases=None, bases_cap=0, out_quals=None, quals_cap=0,
                    out_lens=None, lens_cap=0, out_names=None, names_cap=0, out_name_off=None, off_cap=0, codes=False, base_mode=None, tag=None):
        """rfq_select_rows: the first eight arguments are the rows as rows_to_text / encode_rows take them (d_name_off None: rows without names); d_keep
        n_rows mask bytes (non-zero = keep; None: every row), d_start / d_len n_rows int32 windows (None: 0 / to the end of the read), pairs: rows
        2k / 2k + 1 stand or fall together, min_len: a shorter window drops the row.  out_*: the kept rows at stride row_len, their lengths, name lines
        and n_out + 1 uint64 offsets; no output pointer at all = a size query, an output that is None is not produced.  The bytes are the rows' own.
        tag (None: names are kept whole): a tag of the read's own bases written into the kept names (rfq_name_tag) - a dict of d_tag_start / d_tag_len (n_rows
        int32 each: the part of row i), prefix (bytes, b""), sep (b":"), join (b"_"), at (TAG_AT_SPACE | TAG_AT_END), raw (fields of the struct set as given: the
        tests' refusals); codes / base_mode say what the base rows hold and are looked at only with a tag.
        Returns SelectRowsResult (n_rows, n_bases, names_len, max_len, max_name, n_in, dropped_mask, dropped_short, dropped_mate)."""
        rows = self._rows_in(n_rows, row_len_in, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, codes, 0, base_mode)
        a = A.SelectRowsArgs(d_keep, d_start, d_len, 1 if pairs else 0, min_len, row_len, pad_base, pad_qual, (C.c_uint8 * 2)(),
                             out_bases, bases_cap, out_quals, quals_cap, out_lens, lens_cap, out_names, names_cap, out_name_off, off_cap, None)
        if tag is not None:
            prefix = bytes(tag.get("prefix", b""))
            t = A.NameTag(tag.get("d_tag_start"), tag.get("d_tag_len"), prefix if prefix else None, len(prefix), bytes(tag.get("sep", b":"))[0], bytes(tag.get("join", b"_"))[0],
                          tag.get("at", A.TAG_AT_SPACE), 0)
            self._raw(t, tag.get("raw"))
            a.tag = C.pointer(t)
        return self._call("rfq_select_rows", A.SelectRowsResult, rows, a)

    # --- select_rows with the kept rows grouped by a bin per unit, in one pass (rfq_group_rows)
    def group_rows(self, n_rows, row_len_in, d_bases, d_quals, d_lens, d_names=None, names_len=0, d_name_off=None, d_bin=None, n_bins=1, rest=True, d_keep=None,
                   d_start=None, d_len=None, pairs=False, min_len=1, row_len=0, pad_base=255, pad_qual=255, out_bin_off=None, bin_cap=0, out_bases=None, bases_cap=0,
                   out_quals=None, quals_cap=0, out_lens=None, lens_cap=0, out_names=None, names_cap=0, out_name_off=None, off_cap=0, raw=None):
        """rfq_group_rows: select_rows' arguments and d_bin - one int32 per unit (a row, with pairs the rows 2k / 2k + 1): 0 .. n_bins - 1, below 0 the rest bin
        (rest=True: bin n_bins) or dropped (rest=False); a bin >= n_bins is refused.  The kept rows come out sorted by (bin, input row), stable; out_bin_off:
        n_bins + rest + 1 uint64, the first output row of every bin and the row count last.  No output pointer at all (six of them) = a size query, an output
        that is None is not produced.  raw: fields of the argument struct set as given (the tests' refusals).  Returns GroupRowsResult (select's fields,
        dropped_bin, n_bins_used)."""
        rows = self._rows_in(n_rows, row_len_in, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, False, 0)
        a = A.GroupRowsArgs(d_keep, d_start, d_len, 1 if pairs else 0, min_len, d_bin, n_bins, 1 if rest else 0, out_bin_off, bin_cap, row_len, pad_base, pad_qual,
                            (C.c_uint8 * 2)(), out_bases, bases_cap, out_quals, quals_cap, out_lens, lens_cap, out_names, names_cap, out_name_off, off_cap)
        self._raw(a, raw)
        return self._call("rfq_group_rows", A.GroupRowsResult, rows, a)

    # --- the step that decides: rows -> keep, window, reason and metrics per row (rfq_judge_rows)
    def judge_rows(self, n_rows, row_len, d_bases, d_quals, d_lens, codes=False, trim_front=0, trim_tail=0, poly_g=0, cut_front=False, cut_right=False,
                   cut_tail=False, cut_flags=None, cut_window=0, cut_mean_q=0, max_len=0, min_len=0, max_n=-1, min_mean_q=0, qual_q=0, max_lowq_pct=0,
                   min_complexity_pct=0, d_keep=None, d_start=None, d_len=None, d_why=None, d_metrics=None, base_mode=None):
        """rfq_judge_rows: the rows as rows_to_text takes them (names are not looked at; a quality byte is the score) and the criteria of include/rfq_hip.h:
        trim_front / trim_tail, poly_g, cut_front / cut_right / cut_tail (or cut_flags as bits) with cut_window and cut_mean_q, max_len; then min_len, max_n
        (< 0: off), min_mean_q, qual_q + max_lowq_pct, min_complexity_pct.  d_keep / d_why: n_rows bytes, d_start / d_len: n_rows int32 - what select_rows
        takes -, d_metrics: n_rows x 4 uint32 (qsum, n_cnt, lowq, trans); an output that is None is not produced.  Returns JudgeRowsResult (n_rows, n_kept,
        why_short, why_n, why_meanq, why_lowq, why_complex, bases / qsum / q20 / q30 _in and _out)."""
        rows = self._rows_in(n_rows, row_len, d_bases, d_quals, d_lens, None, 0, None, codes, 0, base_mode)
        flags = cut_flags if cut_flags is not None else (A.CUT_FRONT if cut_front else 0) | (A.CUT_RIGHT if cut_right else 0) | (A.CUT_TAIL if cut_tail else 0)
        a = A.JudgeRowsArgs(trim_front, trim_tail, poly_g, flags, cut_window, cut_mean_q, max_len, min_len, max_n, min_mean_q, qual_q, max_lowq_pct,
                            min_complexity_pct, 0, d_keep, d_start, d_len, d_why, d_metrics)
        return self._call("rfq_judge_rows", A.JudgeRowsResult, rows, a)

    # --- adapter removal, in front of the judge: rows -> the length that is left, the detector, insert sizes (rfq_adapter_rows)
    def adapter_rows(self, n_rows, row_len, d_bases, d_lens, codes=False, pairs=False, min_overlap=0, max_diff=0, max_diff_pct=0, adapter1=None, adapter2=None,
                     adapter_min=0, adapter_mm_per=0, hist_len=0, d_len=None, d_how=None, d_insert=None, d_diff=None, d_insert_hist=None, base_mode=None):
        """rfq_adapter_rows: base rows and lengths (qualities and names are not looked at) and the rules of include/rfq_hip.h: pairs (rows 2k / 2k + 1: the
        overlap search with min_overlap, max_diff, max_diff_pct), adapter1 / adapter2 (bytes of ACGT, at most 64; None: off; adapter2 is the odd rows' with pairs)
        with adapter_min and adapter_mm_per.  d_len: n_rows int32 - what select_rows takes as d_len and a later judge_rows as d_lens -, d_how: n_rows bytes
        (CUT_BY_OVERLAP | CUT_BY_ADAPTER), d_insert / d_diff: n_rows / 2 int32, d_insert_hist: hist_len uint64; an output that is None is not produced.
        Returns AdapterRowsResult (n_rows, n_pairs, pairs_found, rows_cut, rows_cut_overlap, rows_cut_adapter, bases_in, bases_out)."""
        rows = self._rows_in(n_rows, row_len, d_bases, None, d_lens, None, 0, None, codes, 0, base_mode)
        a1 = bytes(adapter1) if adapter1 is not None else None; a2 = bytes(adapter2) if adapter2 is not None else None
        a = A.AdapterRowsArgs(1 if pairs else 0, min_overlap, max_diff, max_diff_pct, a1, len(a1) if a1 else 0, a2, len(a2) if a2 else 0, adapter_min, adapter_mm_per,
                              hist_len, d_len, d_how, d_insert, d_diff, d_insert_hist)
        return self._call("rfq_adapter_rows", A.AdapterRowsResult, rows, a)

    # --- behind the adapter step: every pair with an insert size -> one row, the consensus of both mates (rfq_merge_rows)
    def merge_rows(self, n_rows, row_len_in, d_bases, d_quals, d_lens, d_names=None, names_len=0, d_name_off=None, d_insert=None, codes=False, row_len=0,
                   pad_base=255, pad_qual=255, out_bases=None, bases_cap=0, out_quals=None, quals_cap=0, out_lens=None, lens_cap=0, out_names=None, names_cap=0,
                   out_name_off=None, off_cap=0, base_mode=None):
        """rfq_merge_rows: the first eight arguments are the rows as rows_to_text / encode_rows take them (rows 2k / 2k + 1: R1 / R2; d_name_off None: rows without
        names; a quality byte is the score), d_insert n_rows / 2 int32 - adapter_rows' d_insert: a pair with insert >= 0 becomes one row of insert bases, R1 from the
        front, the reverse complement of R2 from the back, the consensus of include/rfq_hip.h where both cover a position, under R1's name.  out_*: the merged rows at
        stride row_len (up to 2 * row_len_in - 1), their lengths, name lines and n_out + 1 uint64 offsets; no output pointer at all = a size query, an output that
        is None is not produced.  Returns MergeRowsResult (n_rows, n_bases, names_len, max_len, max_name, n_pairs, overlap_bases)."""
        rows = self._rows_in(n_rows, row_len_in, d_bases, d_quals, d_lens, d_names, names_len, d_name_off, codes, 0, base_mode)
        a = A.MergeRowsArgs(d_insert, row_len, pad_base, pad_qual, (C.c_uint8 * 2)(), out_bases, bases_cap, out_quals, quals_cap, out_lens, lens_cap, out_names, names_cap,
                            out_name_off, off_cap)
        return self._call("rfq_merge_rows", A.MergeRowsResult, rows, a)

    # --- between the judge and select_rows: one unit of every class of identical units is kept (rfq_dedup_rows)
    def dedup_rows(self, n_rows, row_len, d_bases, d_quals, d_lens, pairs=False, key_len=0, best_qual=False, mode=None, hist_len=0, d_in=None, d_keep=None,
                   d_dup_of=None, d_count=None, d_hist=None):
        """rfq_dedup_rows: the rows as judge_rows takes them (names are not looked at; d_quals only with best_qual, else it may be None) and the rules of
        include/rfq_hip.h: a unit is a row, or with pairs the rows 2k / 2k + 1; its key the first key_len bases (0: all) of each of its rows, lengths included;
        units with identical keys form a class, of which the lowest unit index - with best_qual the member with the highest score sum over its key, ties to the
        lowest index - is kept.  d_in: n_rows bytes, non-zero = the row is a candidate (judge_rows' d_keep; None: all).  d_keep: n_rows bytes - what select_rows
        takes -, d_dup_of: U int32 (the representative's unit index, -1: no candidate), d_count: U uint32 (the class size at the representative), d_hist: hist_len
        uint64 (bin c - 1: classes of size c, the last bin every larger one); an output that is None is not produced.  mode: the C constant as it stands, for the
        tests of the refusal.  Returns DedupRowsResult (n_units, n_candidates, n_classes, n_dups, max_class, bases_in, bases_kept)."""
        rows = self._rows_in(n_rows, row_len, d_bases, d_quals, d_lens, None, 0, None, False, 0)
        a = A.DedupRowsArgs(1 if pairs else 0, mode if mode is not None else (A.DEDUP_BEST_QUAL if best_qual else A.DEDUP_FIRST), key_len, hist_len, d_in, d_keep,
                            d_dup_of, d_count, d_hist)
        return self._call("rfq_dedup_rows", A.DedupRowsResult, rows, a)

    # --- the report beside the steps that decide: rows under select_rows' triple -> the tables of a QC report (rfq_profile_rows)
    def profile_rows(self, n_rows, row_len, d_bases, d_quals, d_lens, codes=False, pairs=False, d_keep=None, d_start=None, d_len=None, cycles=0, qbins=0, len_bins=0,
                     d_base_cnt=None, d_base_qsum=None, d_qual_hist=None, d_len_hist=None, d_meanq_hist=None, d_gc_hist=None, base_mode=None):
        """rfq_profile_rows: the rows as judge_rows takes them (names are not looked at; a quality byte is the score) and select_rows' triple - d_keep n_rows mask
        bytes (non-zero = counted; None: every row), d_start / d_len n_rows int32 windows (None: 0 / to the end of the read).  With M = 1 + pairs (row i is of mate
        i & 1) the tables, uint64 each: d_base_cnt / d_base_qsum [M][cycles][5] (positions / score sum per cycle and class A C G T other), d_qual_hist
        [M][cycles][qbins], d_len_hist [M][len_bins], d_meanq_hist [M][qbins], d_gc_hist [M][101]; the last row / bin of each collects what lies beyond; a table
        that is None is not produced.  Returns ProfileRowsResult (n_rows, max_len and, per mate, counted, bases, qsum, q20, q30, gc, other)."""
        rows = self._rows_in(n_rows, row_len, d_bases, d_quals, d_lens, None, 0, None, codes, 0, base_mode)
        a = A.ProfileRowsArgs(1 if pairs else 0, cycles, qbins, len_bins, d_keep, d_start, d_len, d_base_cnt, d_base_qsum, d_qual_hist, d_len_hist, d_meanq_hist, d_gc_hist)
        return self._call("rfq_profile_rows", A.ProfileRowsResult, rows, a)

    # --- what a read is: reference sequences -> an index of canonical k-mers, rows against it -> k-mers, hits and a keep byte (rfq_screen_build, rfq_screen_rows)
    def screen_build(self, d_refs, refs_len, d_ref_off, n_refs, k=25, d_index=None, index_cap=0, size_only=False):
        """rfq_screen_build: the references as ASCII bytes back to back on the device (d_refs, refs_len) with n_refs + 1 uint64 offsets (d_ref_off) -> the set of the
        canonical values of their valid k-mers (k in 4 .. 31; a k-mer lies inside one reference and is all ACGT, either case) as an index in the caller's buffer
        d_index (16-byte aligned, index_cap bytes).  size_only: nothing is written, the result says how large the buffer has to be.  Returns ScreenBuildResult
        (n_refs, ref_bases, n_positions, n_kmers, slots, index_bytes)."""
        a = A.ScreenBuildArgs(k, 1 if size_only else 0, d_refs, refs_len, d_ref_off, n_refs, d_index, index_cap)
        return self._call("rfq_screen_build", A.ScreenBuildResult, a)

    def screen_rows(self, n_rows, row_len, d_bases, d_lens, d_index, index_bytes, codes=False, pairs=False, min_hits=1, min_pct=0, keep_matched=False, mode=None,
                    d_in=None, d_kmers=None, d_hits=None, d_keep=None, base_mode=None):
        """rfq_screen_rows: base rows and lengths (qualities and names are not looked at) against an index of screen_build.  A unit is a row, or with pairs the rows
        2u / 2u + 1; d_in: n_rows bytes, non-zero = the row is a candidate (judge_rows' d_keep; None: all).  d_kmers / d_hits: n_rows uint32 - the row's valid
        k-mers and those in the set -, d_keep: n_rows bytes - what dedup_rows takes as d_in and select_rows as d_keep; an output that is None is not produced.  A unit
        matches with H >= max(min_hits, 1) and 100 * H >= min_pct * K over its rows; it is kept when it does not match (keep_matched: when it does).  mode: the C
        constant as it stands, for the tests of the refusal.  Returns ScreenRowsResult (n_units, n_candidates, n_matched, n_kept, kmers, hits, bases_in,
        bases_kept)."""
        rows = self._rows_in(n_rows, row_len, d_bases, None, d_lens, None, 0, None, codes, 0, base_mode)
        a = A.ScreenRowsArgs(1 if pairs else 0, mode if mode is not None else (A.SCREEN_KEEP_MATCHED if keep_matched else A.SCREEN_DROP_MATCHED), min_hits, min_pct,
                             d_index, index_bytes, d_in, d_kmers, d_hits, d_keep)
        return self._call("rfq_screen_rows", A.ScreenRowsResult, rows, a)

    # --- which k-mers the reads hold, and how often: a caller-owned table that adds up across calls, and its reader (rfq_kmers_init, rfq_kmers_rows, rfq_kmers_read)
    def kmers_init(self, k=25, slots=0, d_table=None, table_cap=0, size_only=False):
        """rfq_kmers_init: formats an empty table of canonical k-mers (k in 4 .. 31) with counts in the caller's buffer d_table (16-byte aligned, table_cap bytes):
        S = the power of two >= max(1024, slots) slots, 64 + 16 * S bytes; ask for slots >= 2 x the distinct values expected.  size_only: nothing is written, the
        result says how large the buffer has to be.  Returns KmersInitResult (slots, table_bytes)."""
        a = A.KmersInitArgs(k, 1 if size_only else 0, slots, d_table, table_cap)
        return self._call("rfq_kmers_init", A.KmersInitResult, a)

    def kmers_rows(self, n_rows, row_len, d_bases, d_lens, d_table, table_bytes, codes=False, d_in=None, d_kmers=None, base_mode=None):
        """rfq_kmers_rows: adds 1 to the count of the canonical value of every valid k-mer of every counted row (qualities and names are not looked at) in a table of
        kmers_init; calls on one table add up.  d_in: n_rows bytes, non-zero = the row is counted (judge_rows' d_keep; None: all).  d_kmers: n_rows uint32 - the
        row's valid k-mers, what screen_rows' d_kmers holds - or None.  A table that is too full refuses the call (RFQ_E_NOSPACE) and stays refused until it is
        formatted again.  Returns KmersRowsResult (n_rows, n_counted, bases_in, added, n_new, n_kmers, total, lost)."""
        rows = self._rows_in(n_rows, row_len, d_bases, None, d_lens, None, 0, None, codes, 0, base_mode)
        a = A.KmersRowsArgs(d_table, table_bytes, d_in, d_kmers)
        return self._call("rfq_kmers_rows", A.KmersRowsResult, rows, a)

    def kmers_read(self, d_table, table_bytes, min_count=1, max_count=0, size_only=False, hist_len=0, d_hist=None, d_values=None, d_counts=None, list_cap=0,
                   d_index=None, index_cap=0):
        """rfq_kmers_read: what a table of kmers_init / kmers_rows holds.  An entry is selected when max(min_count, 1) <= count and (max_count == 0 or count <=
        max_count).  d_hist: hist_len uint64, bin c - 1 = the distinct values with count c over all entries, the last bin every larger count (the k-mer spectrum);
        d_values / d_counts: list_cap uint64 each, the selected entries in an unspecified order; d_index (16-byte aligned, index_cap bytes): a screen index of the
        selected values, which screen_rows takes; an output that is None is not produced.  size_only: nothing is written.  Returns KmersReadResult (k, slots,
        n_kmers, total, max_count, n_selected, selected_total, index_slots, index_bytes)."""
        a = A.KmersReadArgs(d_table, table_bytes, min_count, max_count, 1 if size_only else 0, hist_len, d_hist, d_values, d_counts, list_cap, d_index, index_cap)
        return self._call("rfq_kmers_read", A.KmersReadResult, a)

    # --- whose read is this: rows against one or two sets of barcodes (rfq_demux_rows)
    @staticmethod
    def _barcode_set(barcodes, length=None):
        """(n, len, the [n][len] bytes) of a list of str / bytes of one length, or of bytes already laid out with `length` given"""
        if barcodes is None:
            return 0, 0, None
        if isinstance(barcodes, (bytes, bytearray)):
            assert length, "barcodes as one bytes object need their length"
            return len(barcodes) // length, length, bytes(barcodes)
        bcs = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
        ln = length if length is not None else (len(bcs[0]) if bcs else 0)
        assert all(len(b) == ln for b in bcs), "the barcodes of a set have one length"
        return len(bcs), ln, b"".join(bcs)

    def demux_rows(self, n_rows, row_len, d_bases, d_lens, barcodes1, barcodes2=None, sheet=None, codes=False, pairs=False, off1=0, off2=0, skip1=0, skip2=0,
                   max_mm=1, min_delta=1, d_in=None, d_sample=None, d_why=None, d_best=None, d_dist=None, d_keep=None, d_start=None, d_counts=None, base_mode=None,
                   raw=None):
        """rfq_demux_rows: base rows and lengths (qualities and names are not looked at) against one or two sets of barcodes.  barcodes1 / barcodes2: a list of str
        / bytes of one length (A C G T in either case), read at [off, off + len) of row u / of rows 2u and 2u + 1 with pairs; sheet: a list of (i, j) pairs, sample
        s the pair listed s-th (None: every combination, i * n2 + j).  A row matches its set with d1 <= max_mm and d2 - d1 >= min_delta (Hamming distances of the
        best and the second best barcode; an N never agrees).  d_in: n_rows bytes, non-zero = the row is a candidate.  d_sample [U] int32, d_why [U] uint8, d_best
        [n_rows] int32, d_dist [n_rows] uint8, d_keep [n_rows] uint8 and d_start [n_rows] int32 - what select_rows takes -, d_counts [n_samples + 1] uint64; an
        output that is None is not produced.  raw: a dict of DemuxRowsArgs fields set as they stand, for the tests of the refusals.  Returns DemuxRowsResult
        (n_units, n_candidates, n_assigned, n_samples, n_exact, why_none, why_ambig, why_short, why_combo, bases_in, bases_out)."""
        rows = self._rows_in(n_rows, row_len, d_bases, None, d_lens, None, 0, None, codes, 0, base_mode)
        n1, len1, b1 = self._barcode_set(barcodes1)
        n2, len2, b2 = self._barcode_set(barcodes2)
        flat = None
        if sheet is not None:
            flat = (C.c_int32 * max(2 * len(sheet), 1))(*[int(x) for p in sheet for x in p])
        a = A.DemuxRowsArgs(1 if pairs else 0, n1, len1, off1, skip1, b1, n2, len2, off2, skip2, b2, flat, len(sheet) if sheet is not None else 0, max_mm, min_delta,
                            d_in, d_sample, d_why, d_best, d_dist, d_keep, d_start, d_counts)
        self._raw(a, raw)
        return self._call("rfq_demux_rows", A.DemuxRowsResult, rows, a)

    # --- --compare on the device: first offset at which two device texts differ (n when identical)
    def first_diff(self, d_a, d_b, n) -> int:
        out = C.c_uint64(0)
        self._check(self._L.rfq_compare_bytes(self._h, d_a, d_b, n, C.byref(out)))
        return out.value

    def timings(self):
        names = (C.c_char_p * 32)(); ms = (C.c_float * 32)()
        n = self._L.rfq_last_timings(self._h, names, ms, 32)
        return [(names[i].decode(), ms[i]) for i in range(n)]

    # --- host-bytes conveniences (tests, small tools)
    def dev_put(self, data: bytes):
        p = C.c_void_p()
        self._check(self._L.rfq_dev_malloc(self._h, C.byref(p), max(len(data), 1) + 64))
        self._check(self._L.rfq_copy_h2d(self._h, p, data, len(data)))
        return p

    def dev_get(self, d_ptr, n) -> bytes:
        buf = C.create_string_buffer(max(n, 1))
        self._check(self._L.rfq_copy_d2h(self._h, buf, d_ptr, n))
        return buf.raw[:n]

    def dev_free(self, p):
        self._L.rfq_dev_free(self._h, p)

    def encode_bytes(self, fq1: bytes, fq2: bytes = b"", paired=SE, chunk_bases=1_000_000, **kw) -> bytes:
        d1 = self.dev_put(fq1); d2 = self.dev_put(fq2) if paired == PE_TWO_FILES else None
        try:
            r = self.encode(d1, len(fq1), d2, len(fq2) if d2 else 0, paired, chunk_bases, **kw)
            return self.dev_get(r.d_rfq, r.rfq_len) if r.rfq_len else b""
        finally:
            self.dev_free(d1)
            if d2:
                self.dev_free(d2)

    def decode_bytes(self, rfq: bytes, split_pe=False, out_caps=None, **kw):
        """out_caps = (cap1, cap2): decode into buffers of the caller (allocated here, of those sizes) instead of the context's own result buffers - the path a
        pipelined host takes (rfq_decode_args.d_out1 / d_out2), on which the emitter is launched ahead of the host's look at the status."""
        d = self.dev_put(rfq); o1 = o2 = None
        try:
            if out_caps is not None:
                o1 = self.dev_put(b"\0" * max(int(out_caps[0]), 1)); o2 = self.dev_put(b"\0" * max(int(out_caps[1]), 1)) if split_pe else None
                kw = dict(kw, d_out1=o1, cap1=int(out_caps[0]), d_out2=o2, cap2=int(out_caps[1]) if split_pe else 0)
            r = self.decode(d, len(rfq), split_pe=split_pe, **kw)
            a = self.dev_get(r.d_fq1, r.n1) if r.n1 else b""
            b = self.dev_get(r.d_fq2, r.n2) if (split_pe and r.n2) else b""
            return (a, b) if split_pe else a
        finally:
            self.dev_free(d)
            if o1 is not None: self.dev_free(o1)
            if o2 is not None: self.dev_free(o2)


def nolb_threshold(file_size: int, ends_with_newline: bool) -> int:
    """Offset from which the reference's reader has its "no line break at the end" flag up (src/fastqreader.cpp:31-46):
    the start of its final, short 1 MiB block when the file lacks a trailing newline.  A file of exactly k MiB has no short block: the
    flag goes up at the empty read behind the last full block - whatever the last byte is (the test reads the byte in front of the
    buffer there: never a line break in practice) - so the threshold is the file size itself: it is met by an unterminated last record
    and by the readers' last, failed attempt, i.e. by the input's tail chunk."""
    if file_size == 0:
        return U64_MAX
    if file_size % (1 << 20) == 0:
        return file_size
    if ends_with_newline:
        return U64_MAX
    return ((file_size - 1) >> 20) << 20
