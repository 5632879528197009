"""rfq_judge_rows against the torch recipe for the same outputs, on one context, one process (configs[2]-shaped rows: fastq_to_tensors of synthetic NovaSeq PE150
in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 2.8 M reads at row_len 160: the recipe's int32
intermediates are sixteen times the rows).  Criteria: cut_tail (window 4, mean 20) + max_n + min_mean_q + qual_q / max_lowq_pct + min_len.  Warmed up,
alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.judge_rows: the output tensors and the call (keep, start, length, why and the summary)
  (b) the same keep / start / length / why in torch: the scores as int32 under a length mask, cumsum along the row, window sums by a shifted difference, the last
      good start by a masked max, the counts by masked sums - checked equal to (a) once before timing
Beside them, not gated: a device-to-device copy of the bytes (a) reads and writes (its ceiling).
One JSON line: ms (median, min, all), the stage, a over b, the copy's share of (a).  Exit status 0 when the median of (a) is below the median of (b).
    python tools/judge_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_800_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, judge_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    fastq_bytes = t1.numel() + t2.numel()
    del a1, a2
    L = args.row_len
    t = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L)
    del t1, t2
    n = t["lens"].numel()
    assert n == 2 * args.pairs
    W, MQ, MIN_LEN, MAX_N, MEAN, QUAL_Q, PCT = 4, 20, 36, 2, 25, 15, 20
    crit = dict(cut_tail=True, cut_window=W, cut_mean_q=MQ, min_len=MIN_LEN, max_n=MAX_N, min_mean_q=MEAN, qual_q=QUAL_Q, max_lowq_pct=PCT)
    res = {}

    def run_a():
        res["a"] = judge_rows(codec, t, **crit)
        return codec.timings()

    def run_b():
        bases, quals, lens = t["bases"], t["quals"], t["lens"]
        pos = torch.arange(L, device=dev, dtype=torch.int32)
        inside = pos[None, :] < lens[:, None]
        q = torch.where(inside, quals.to(torch.int32), 0)
        P = torch.nn.functional.pad(q.cumsum(1, dtype=torch.int32), (1, 0))                        # [n, L + 1]: P[:, i] = the sum of the first i scores
        w = torch.clamp(lens, max=W)                                                              # (a read shorter than the window has one window: itself)
        hi = torch.gather(P, 1, (pos[None, :] + w[:, None]).clamp_(max=L).long())
        good = ((hi - P[:, :L]) >= MQ * w[:, None]) & (pos[None, :] <= (lens - w)[:, None]) & (lens > 0)[:, None]
        last = torch.where(good, pos[None, :], -1).amax(1)
        length = torch.where(last >= 0, last + w, 0).to(torch.int32)
        win = pos[None, :] < length[:, None]
        qsum = torch.gather(P, 1, length[:, None].long())[:, 0]
        n_cnt = ((bases == 4) & win).sum(1, dtype=torch.int32); lowq = ((quals < QUAL_Q) & win).sum(1, dtype=torch.int32)
        why = (length < MIN_LEN).to(torch.uint8) | ((n_cnt > MAX_N).to(torch.uint8) << 1) | ((qsum < MEAN * length).to(torch.uint8) << 2) | \
            ((lowq * 100 > PCT * length).to(torch.uint8) << 3)
        res["b"] = {"keep": (why == 0).to(torch.uint8), "start": torch.zeros_like(length), "length": length, "why": why}
        return []

    # the ceiling: a copy of k bytes reads k and writes k.  (a) reads both row arrays and a length per row; it writes a keep and a reason byte, a start and a length
    traffic = (2 * n * L + 4 * n) + n * (1 + 1 + 4 + 4)
    scratch = torch.empty(traffic // 2, dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

    def run_copy():
        scratch2.copy_(scratch)
        return []
    runs = {"a_judge_rows": run_a, "b_torch_recipe": run_b, "copy_ceiling": run_copy}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    for k in ("keep", "start", "length", "why"):                             # the two sides make the same tensors
        assert res["a"][k].dtype == res["b"][k].dtype and torch.equal(res["a"][k], res["b"][k]), k
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
    out = {"tool": "judge_bench", "workload": "rows of synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d) at row_len %d; cut_tail window %d mean %d, "
           "min_len %d, max_n %d, min_mean_q %d, qual_q %d at most %d %%" % (fastq_bytes / 2e9, args.pairs, args.seed, L, W, MQ, MIN_LEN, MAX_N, MEAN, QUAL_Q, PCT),
           "rows": n, "traffic_bytes": traffic, "reps": args.reps, "summary": summary}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    out["a_over_b"] = round(out["a_judge_rows"]["ms_median"] / out["b_torch_recipe"]["ms_median"], 4)
    out["copy_share_of_a"] = round(out["copy_ceiling"]["ms_median"] / max(out["a_judge_rows"]["ms_median"], 1e-9), 3)
    out["copy_share_of_kernel"] = round(out["copy_ceiling"]["ms_median"] / max(out["a_judge_rows"]["stages_ms"].get("judge:rows", 0.0), 1e-9), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0 if out["a_judge_rows"]["ms_median"] < out["b_torch_recipe"]["ms_median"] else 1


if __name__ == "__main__":
    sys.exit(main())
