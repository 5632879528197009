"""rfq_adapter_rows beside rfq_judge_rows and a copy, on one context, one process.  The rows are made with torch on the device: fragments of 60 .. 500 bases cut
from a fixed pseudo-genome (codes), read from both ends as reads of 150 at row_len 160 - the fragment, then the adapter, then noise -, with --err substitutions
per base; --pairs sets the size (default 1.4 M pairs = 2.8 M rows).  Before timing, the first 4096 pairs are checked against the host loop of tests/_adapter.py.
Warmed up, alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.trim_adapters, pairs + both adapters + a histogram of 512 bins, with its defaults
  (b) repaq_amd.tensors.judge_rows on the same rows with the criteria of tools/judge_bench.py
  (c) a device-to-device copy of the base rows (what (a) has to read at the least)
One JSON line: ms (median, min, all), the adapter:rows stage, a over b, the copy's share of (a).
    python tools/adapter_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

AD1, AD2 = b"AGATCGGAAGAGC", b"CTGTCTCTTATAC"


def make_rows(torch, dev, pairs, L, read, seed, err):
    """(bases [2 pairs, L] codes, quals, lens, inserts [pairs]) on the device, in slices of 2^17 pairs"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    genome = torch.randint(0, 4, (1 << 22,), generator=g, device=dev, dtype=torch.uint8)
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    ads = [torch.tensor([code[c] for c in a], dtype=torch.uint8, device=dev) for a in (AD1, AD2)]
    bases = torch.empty((2 * pairs, L), dtype=torch.uint8, device=dev); inserts = torch.empty((pairs,), dtype=torch.int64, device=dev)
    pos = torch.arange(L, device=dev)[None, :]
    for k0 in range(0, pairs, 1 << 17):
        k = min(1 << 17, pairs - k0)
        ins = torch.randint(60, 501, (k, 1), generator=g, device=dev); start = torch.randint(0, (1 << 22) - 512, (k, 1), generator=g, device=dev)
        inserts[k0:k0 + k] = ins[:, 0]
        for m in (0, 1):
            inside = pos < ins
            at = torch.where(inside, start + pos, start) if m == 0 else torch.where(inside, start + ins - 1 - pos, start)
            b = genome[at]
            if m == 1:
                b = 3 - b
            flip = torch.rand((k, L), generator=g, device=dev) < err
            b = torch.where(flip, (b + torch.randint(1, 4, (k, L), generator=g, device=dev, dtype=torch.uint8)) & 3, b)
            ai = (pos - ins).clamp_(0, len(AD1) - 1)
            b = torch.where((pos >= ins) & (pos < ins + len(AD1)), ads[m][ai], b)
            b = torch.where(pos >= ins + len(AD1), torch.randint(0, 4, (k, L), generator=g, device=dev, dtype=torch.uint8), b)
            b = torch.where(pos >= read, torch.full_like(b, 255), b)
            bases[2 * k0 + m:2 * (k0 + k):2] = b
    quals = torch.randint(12, 41, (2 * pairs, L), generator=g, device=dev, dtype=torch.uint8)
    lens = torch.full((2 * pairs,), read, dtype=torch.int32, device=dev)
    return bases, quals, lens, inserts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_400_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--read", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.003)
    ap.add_argument("--check", type=int, default=4096)
    args = ap.parse_args()
    import numpy as np
    import torch
    import _adapter as A
    from repaq_amd import RfqCodec
    from repaq_amd.tensors import trim_adapters, judge_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    L = args.row_len
    bases, quals, lens, inserts = make_rows(torch, dev, args.pairs, L, args.read, args.seed, args.err)
    t = {"bases": bases, "quals": quals, "lens": lens}
    n = 2 * args.pairs
    HIST = 512
    crit_a = dict(pairs=True, adapter1=AD1, adapter2=AD2, hist_len=HIST)
    crit_j = dict(cut_tail=True, cut_window=4, cut_mean_q=20, min_len=36, max_n=2, min_mean_q=25, qual_q=15, max_lowq_pct=20)
    # the first pairs against the host loop, with trim_adapters' defaults written out
    nc = min(args.check, args.pairs)
    head = {"bases": bases[:2 * nc].contiguous(), "lens": lens[:2 * nc].contiguous()}
    got = trim_adapters(codec, head, **crit_a)
    want = A.expected(head["bases"].cpu().numpy(), head["lens"].cpu().numpy(), A.crit(pairs=True, min_overlap=30, max_diff=5, max_diff_pct=20, adapter1=AD1, adapter2=AD2,
                                                                                   adapter_min=4, adapter_mm_per=8, hist_len=HIST), True)
    for k, w in (("length", "length"), ("how", "how"), ("insert", "insert"), ("diff", "diff"), ("insert_hist", "hist")):
        assert np.array_equal(got[k].cpu().numpy().astype(np.int64), want[w].astype(np.int64)), k
    assert got["summary"] == want["summary"]
    true_ins = inserts[:nc].cpu().numpy(); found = want["insert"]
    short = true_ins <= 2 * args.read - 30
    recovered = int(((found == true_ins) & short).sum())
    res = {}

    def run_a():
        res["a"] = trim_adapters(codec, t, **crit_a)
        return codec.timings()

    def run_j():
        res["j"] = judge_rows(codec, t, **crit_j)
        return codec.timings()
    scratch = torch.empty_like(bases)

    def run_copy():
        scratch.copy_(bases)
        return []
    runs = {"a_trim_adapters": run_a, "b_judge_rows": run_j, "copy_of_the_base_rows": run_copy}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    summary = res["a"]["summary"]
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            res.clear()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for name, v in st:
                stages[k][name] = stages[k].get(name, 0.0) + v / args.reps
    out = {"tool": "adapter_bench", "workload": "%d pairs of reads of %d at row_len %d (codes) from fragments of 60 .. 500 bases of a pseudo-genome, adapter and noise behind the "
           "fragment, %.3f substitutions per base, seed %d; trim_adapters' defaults (min_overlap 30, max_diff 5, max_diff_pct 20, adapter_min 4, adapter_mm_per 8), both "
           "adapters, %d histogram bins" % (args.pairs, args.read, L, args.err, args.seed, HIST),
           "rows": n, "reps": args.reps, "checked_pairs": nc, "checked_short_inserts": int(short.sum()), "checked_short_inserts_recovered": recovered, "summary": summary}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    out["a_over_b"] = round(out["a_trim_adapters"]["ms_median"] / out["b_judge_rows"]["ms_median"], 3)
    out["kernel_over_judge_kernel"] = round(out["a_trim_adapters"]["stages_ms"].get("adapter:rows", 0.0) / max(out["b_judge_rows"]["stages_ms"].get("judge:rows", 0.0), 1e-9), 3)
    out["copy_share_of_a"] = round(out["copy_of_the_base_rows"]["ms_median"] / max(out["a_trim_adapters"]["ms_median"], 1e-9), 3)
    out["copy_share_of_kernel"] = round(out["copy_of_the_base_rows"]["ms_median"] / max(out["a_trim_adapters"]["stages_ms"].get("adapter:rows", 0.0), 1e-9), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
