"""rfq_decode_names against the full text decode on one context, one process (configs[2]-shaped input: synthetic NovaSeq PE150, 2 x 4 GB, -k 1000,
fqgen profile 1, seed 3 - bench.py's generator path; an SE150 image of the same number of reads as a second line).  Each image is encoded once; then,
warmed up, alternating and repeated, timed with device events:
  (a) rfq_decode_batch (split_pe = 0) without a chunk index, context-owned text
  (b) rfq_decode_names without a chunk index, context-owned names and offsets
One JSON line per image: ms (median, min, all), the stages of rfq_last_timings, names/s, the bytes (b) writes (names + offsets) per name byte, b over a.
    python tools/names_bench.py [--pairs N] [--reps K]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(codec, torch, dev, label, workload, t1, t2, paired, args):
    r = codec.encode(t1.data_ptr(), t1.numel(), t2.data_ptr() if t2 is not None else None, t2.numel() if t2 is not None else 0, paired, 1_000_000)
    rfq = torch.empty(r.rfq_len, dtype=torch.uint8, device=dev)
    codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(rfq.data_ptr()), C.c_void_p(r.d_rfq), r.rfq_len))
    text_bytes = t1.numel() + (t2.numel() if t2 is not None else 0)
    res = {}

    def run_text():
        res["a_text"] = codec.decode(rfq.data_ptr(), rfq.numel(), split_pe=False)

    def run_names():
        res["b_names"] = codec.decode_names(rfq.data_ptr(), rfq.numel())
    runs = {"a_text": run_text, "b_names": run_names}
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
    assert res["a_text"].n1 == text_bytes, (res["a_text"].n1, text_bytes)
    n = int(res["b_names"].n_rows); nb = int(res["b_names"].names_len)
    out = {"tool": "names_bench", "image": label, "workload": workload, "rfq_bytes": int(r.rfq_len), "fastq_bytes": text_bytes, "rows": n, "name_bytes": nb,
           "max_name": int(res["b_names"].max_name), "reps": args.reps}
    for k, v in ms.items():
        s = sorted(v); med = s[len(s) // 2]
        ob = text_bytes if k == "a_text" else nb + 8 * (n + 1)
        out[k] = {"ms_median": round(med, 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "rows_per_s": round(n / (med / 1e3)),
                  "output_bytes": ob, "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    out["b_names"]["bytes_written_per_name_byte"] = round((nb + 8 * (n + 1)) / max(nb, 1), 4)
    out["b_over_a"] = round(out["b_names"]["ms_median"] / out["a_text"]["ms_median"], 4)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11_200_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES, SE
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    pe = measure(codec, torch, dev, "pe150", "synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d), -k 1000" % (t1.numel() / 1e9, args.pairs, args.seed),
                 t1, t2, PE_TWO_FILES, args)
    del t1, t2
    codec.clearHeader()
    s1, _ = O.gen_np(O.NOVA_SE150, 2 * args.pairs, seed=args.seed)
    t1 = torch.from_numpy(s1).to(dev)
    del s1
    se = measure(codec, torch, dev, "se150", "synthetic NovaSeq SE150 %.2f GB (%d reads, seed %d), -k 1000" % (t1.numel() / 1e9, 2 * args.pairs, args.seed), t1, None, SE, args)
    codec.close()
    return 0 if pe["b_over_a"] < 1.0 and se["b_over_a"] < 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
