"""rfq_decode_rows against the text decode on one context (configs[2]-shaped input: synthetic NovaSeq PE150, 2 x 4 GB, -k 1000, fqgen profile 1,
seed 3 - bench.py's generator path).  The image is encoded once; then, warmed up, alternating and repeated, timed with device events:
  (a) rfq_decode_batch without a chunk index into caller buffers (split_pe = 1, as bench.py decodes)
  (b) rfq_decode_rows, row_len 160, codes, into preallocated buffers
  (c) the same with row_len 150
One JSON line: ms (median, min), rows/s, output bytes, and the HBM bytes of the outputs per FASTQ byte.
    python tools/rows_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11_200_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    n1, n2 = int(a1.size), int(a2.size)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    r = codec.encode(t1.data_ptr(), n1, t2.data_ptr(), n2, PE_TWO_FILES, 1_000_000)
    rfq = torch.empty(r.rfq_len, dtype=torch.uint8, device=dev)
    import ctypes as C
    codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(rfq.data_ptr()), C.c_void_p(r.d_rfq), r.rfq_len))
    del t1, t2
    o1 = torch.empty(n1 + 64, dtype=torch.uint8, device=dev); o2 = torch.empty(n2 + 64, dtype=torch.uint8, device=dev)
    q = codec.decode_rows(rfq.data_ptr(), rfq.numel())
    n = int(q.n_rows)
    bufs = {L: (torch.empty((n, L), dtype=torch.uint8, device=dev), torch.empty((n, L), dtype=torch.uint8, device=dev)) for L in (160, 150)}
    lens = torch.empty(n, dtype=torch.int32, device=dev)

    def run_a():
        codec.decode(rfq.data_ptr(), rfq.numel(), split_pe=True, d_out1=o1.data_ptr(), cap1=n1 + 64, d_out2=o2.data_ptr(), cap2=n2 + 64)

    def run_rows(L):
        b, qq = bufs[L]
        codec.decode_rows(rfq.data_ptr(), rfq.numel(), row_len=L, codes=True, d_bases=b.data_ptr(), bases_cap=n * L, d_quals=qq.data_ptr(),
                          quals_cap=n * L, d_lens=lens.data_ptr(), lens_cap=n)
    runs = {"a_text": run_a, "b_rows160": lambda: run_rows(160), "c_rows150": lambda: run_rows(150)}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for name, t in codec.timings():
                stages[k][name] = stages[k].get(name, 0.0) + t / args.reps
    text_bytes = n1 + n2
    out = {"tool": "rows_bench", "workload": "configs[2]: synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d), -k 1000" % (n1 / 1e9, args.pairs, args.seed),
           "rfq_bytes": int(r.rfq_len), "fastq_bytes": text_bytes, "rows": n, "bases": int(q.n_bases), "max_len": int(q.max_len), "reps": args.reps}
    for k, v in ms.items():
        s = sorted(v); med = s[len(s) // 2]
        ob = text_bytes if k == "a_text" else n * (160 if "160" in k else 150) * 2 + 4 * n
        out[k] = {"ms_median": round(med, 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "rows_per_s": round(n / (med / 1e3)),
                  "output_bytes": ob, "output_bytes_per_fastq_byte": round(ob / text_bytes, 4), "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    out["b_over_a"] = round(out["b_rows160"]["ms_median"] / out["a_text"]["ms_median"], 3)
    print(json.dumps(out), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
