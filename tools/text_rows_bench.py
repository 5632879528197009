"""rfq_text_rows against the route through the codec, on one context, one process (configs[2]-shaped input: synthetic NovaSeq PE150 in two files,
fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 4 GB).  Warmed up, alternating and repeated, timed
with device events:
  (a) rfq_text_rows: all five outputs, codes, row_len 160, into caller buffers
  (b) the same result without it: rfq_encode_batch -> rfq_decode_rows (codes, row_len 160, caller buffers) + rfq_decode_names; the image is copied
      out of the context's result buffer into a buffer allocated once up front (part of (b); timed alone as copy_image, and a over b is also given
      with that copy taken off (b))
Beside them, not gated: a device-to-device copy of the bytes each writer reads and writes (its ceiling), and the line index as a share of (a).
One JSON line: ms (median, min, all), the stages of rfq_last_timings, a over b.  Exit status 0 when (a) is faster than (b).
    python tools/text_rows_bench.py [--pairs N] [--reps K]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11_200_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    L = args.row_len
    src = dict(d_fq2=t2.data_ptr(), n2=t2.numel(), paired=PE_TWO_FILES)
    q = codec.text_rows(t1.data_ptr(), t1.numel(), **src)
    n, nl = int(q.n_rows), int(q.names_len)
    assert n == 2 * args.pairs and q.max_len <= L and (q.consumed1, q.consumed2) == (t1.numel(), t2.numel())
    bases = torch.empty((n, L), dtype=torch.uint8, device=dev); quals = torch.empty((n, L), dtype=torch.uint8, device=dev)
    lens = torch.empty((n,), dtype=torch.int32, device=dev); blob = torch.empty((nl,), dtype=torch.uint8, device=dev); off = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    rows_out = dict(row_len=L, codes=True, d_bases=bases.data_ptr(), bases_cap=n * L, d_quals=quals.data_ptr(), quals_cap=n * L, d_lens=lens.data_ptr(), lens_cap=n)
    res = {}

    def run_a():
        res["a"] = codec.text_rows(t1.data_ptr(), t1.numel(), d_names=blob.data_ptr(), names_cap=nl, d_name_off=off.data_ptr(), off_cap=n + 1, **rows_out, **src)
        return [codec.timings()]

    keep = torch.empty(t1.numel() + t2.numel(), dtype=torch.uint8, device=dev)       # (b)'s image: never larger than the text
    image_bytes = {}

    def run_b():
        codec.clearHeader()
        e = codec.encode(t1.data_ptr(), t1.numel(), t2.data_ptr(), t2.numel(), PE_TWO_FILES, 1_000_000)
        st = [codec.timings()]
        # (the image leaves the context's result buffer, which the next call on the context may reuse, for a buffer of the caller's allocated once up front: that
        # device-to-device copy is part of (b) and is also timed alone, as copy_image)
        img_n = e.rfq_len
        assert img_n <= keep.numel()
        codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(keep.data_ptr()), C.c_void_p(e.d_rfq), img_n))
        res["b_rows"] = codec.decode_rows(keep.data_ptr(), img_n, **rows_out); st.append(codec.timings())
        image_bytes["n"] = int(img_n)
        res["b_names"] = codec.decode_names(keep.data_ptr(), img_n, d_names=blob.data_ptr(), names_cap=nl, d_name_off=off.data_ptr(), off_cap=n + 1); st.append(codec.timings())
        return st

    # ceilings: a device-to-device copy of the bytes a writer reads and writes (the rows writer: the sequence and quality lines in, two row arrays out; the
    # names writer: the name lines in, the blob out) - a copy of k bytes reads k and writes k, so it stands for 2 k bytes of traffic
    n_bases = int(q.n_bases)
    rows_bytes = (2 * n_bases + 2 * n * L) // 2; names_bytes = nl
    scratch = torch.empty(max(rows_bytes, names_bytes, 1), dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

    def run_copy(k):
        scratch2[:k].copy_(scratch[:k])
        return []
    runs = {"a_text_rows": run_a, "b_codec_route": run_b, "copy_rows": lambda: run_copy(rows_bytes), "copy_names": lambda: run_copy(names_bytes),
            "copy_image": lambda: run_copy(min(image_bytes.get("n", 0), scratch.numel()))}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for call in st:
                for name, t in call:
                    stages[k][name] = stages[k].get(name, 0.0) + t / args.reps
    assert res["b_rows"].n_rows == n and res["b_names"].n_rows == n and res["a"].n_rows == n
    out = {"tool": "text_rows_bench", "workload": "synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d), rows of %d, codes" % (t1.numel() / 1e9, args.pairs, args.seed, L),
           "fastq_bytes": t1.numel() + t2.numel(), "rows": n, "bases": n_bases, "name_bytes": nl, "reps": args.reps}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    a = out["a_text_rows"]
    out["image_bytes"] = image_bytes.get("n", 0)
    out["a_over_b"] = round(a["ms_median"] / out["b_codec_route"]["ms_median"], 4)
    out["a_over_b_less_image_copy"] = round(a["ms_median"] / max(out["b_codec_route"]["ms_median"] - out["copy_image"]["ms_median"], 1e-9), 4)
    out["rows_writer_over_copy"] = round(a["stages_ms"].get("text_rows:rows", 0.0) / max(out["copy_rows"]["ms_median"], 1e-9), 3)
    out["names_writer_over_copy"] = round(a["stages_ms"].get("text_rows:names", 0.0) / max(out["copy_names"]["ms_median"], 1e-9), 3)
    out["index_share_of_a"] = round(a["stages_ms"].get("index", 0.0) / max(a["ms_median"], 1e-9), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0 if out["a_over_b"] < 1.0 and out["a_over_b_less_image_copy"] < 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
