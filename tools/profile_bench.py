"""rfq_profile_rows against the torch recipe for the same tables, on one context, one process (configs[2]-shaped rows: fastq_to_tensors of synthetic NovaSeq PE150
in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160).  Pairs, codes, all six
tables, cycles = row_len, 64 score bins.  Two workloads: "before" (the raw rows) and "after" (under the keep / start / length the judge leaves for a quality trim and
filter).  Warmed up, alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.profile_rows: the output tensors and the call, with its stage time profile:rows
  (b) the same tables in torch: a window mask over [n, L], the cell index of every position (mate, cycle, class / score bin) and bincount over the masked
      positions - with the scores as weights for the score sums -, the per-read bins from row sums and bincount - checked equal to (a) once before timing
Beside them, not gated: a device-to-device copy of the bytes (a) reads from the rows (its ceiling), and the judge:rows stage of rfq_judge_rows on the same rows,
which reads the same bytes.
One JSON line per workload: ms (median, min, all), the stages, a over b, bytes of rows / time of (a) against the HBM peak DESIGN.md §5 uses (8 TB/s).  No ratio is
fixed in advance: exit status 0 when every line was produced and (a) equals (b).
    python tools/profile_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8e12
TABLES = ("base_cnt", "base_qsum", "qual_hist", "len_hist", "meanq_hist", "gc_hist")
JUDGE = dict(cut_tail=True, cut_window=4, cut_mean_q=20, poly_g=10, max_n=5, min_mean_q=20, qual_q=15, max_lowq_pct=40, min_len=36)


def torch_recipe(torch, t, keep, start, length, L, qbins):
    """the six tables of profile_rows(pairs=True, codes=True, cycles=L, len_bins=L + 1) from torch ops"""
    bases, quals, lens = t["bases"], t["quals"], t["lens"]
    n = lens.numel(); dev = bases.device
    a = start.long() if start is not None else torch.zeros(n, dtype=torch.int64, device=dev)
    w = length.long() if length is not None else lens.long() - a
    if keep is not None:
        w = torch.where(keep != 0, w, torch.full_like(w, -1))               # (a dropped row has no position and no bin)
    pos = torch.arange(L, device=dev)[None, :]
    inside = (pos >= a[:, None]) & (pos < (a + w)[:, None])
    mate = (torch.arange(n, device=dev) & 1)[:, None]
    cyc = (pos - a[:, None]).clamp(0, L - 1)
    cls = bases.long().clamp(max=4); q = quals.long()
    cell = ((mate * L + cyc) * 5 + cls)[inside]; qv = q[inside]
    out = {"base_cnt": torch.bincount(cell, minlength=2 * L * 5).view(2, L, 5),
           "base_qsum": torch.bincount(cell, weights=qv.double(), minlength=2 * L * 5).long().view(2, L, 5),
           "qual_hist": torch.bincount(((mate * L + cyc) * qbins + q.clamp(max=qbins - 1))[inside], minlength=2 * L * qbins).view(2, L, qbins)}
    counted = w >= 0; m1 = mate[:, 0]
    qsum = (q * inside).sum(1); acgt = ((cls < 4) & inside).sum(1); gc = (((cls == 1) | (cls == 2)) & inside).sum(1)
    out["len_hist"] = torch.bincount((m1 * (L + 1) + w.clamp(0, L))[counted], minlength=2 * (L + 1)).view(2, L + 1)
    has = counted & (w > 0)
    out["meanq_hist"] = torch.bincount((m1 * qbins + (qsum // w.clamp(min=1)).clamp(max=qbins - 1))[has], minlength=2 * qbins).view(2, qbins)
    hasb = counted & (acgt > 0)
    out["gc_hist"] = torch.bincount((m1 * 101 + 100 * gc // acgt.clamp(min=1))[hasb], minlength=202).view(2, 101)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--qbins", type=int, default=64)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, judge_rows, profile_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    fastq_bytes = t1.numel() + t2.numel()
    del a1, a2
    L = args.row_len
    t = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L, names=False)
    del t1, t2
    n = t["lens"].numel()
    j = judge_rows(codec, t, **JUDGE)
    rc = 0
    for label, triple in (("before", dict(keep=None, start=None, length=None)), ("after", dict(keep=j["keep"], start=j["start"], length=j["length"]))):
        res = {}

        def run_a():
            res["a"] = profile_rows(codec, t, pairs=True, qbins=args.qbins, **triple)
            return codec.timings()

        def run_b():
            res["b"] = torch_recipe(torch, t, triple["keep"], triple["start"], triple["length"], L, args.qbins)
            return []

        def run_judge():
            judge_rows(codec, t, **JUDGE)
            return codec.timings()
        traffic = 2 * n * L + 4 * n + (9 * n if triple["keep"] is not None else 0)      # (a) reads both row buffers and a length per row, and the triple
        scratch = torch.empty(traffic, dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

        def run_copy():
            scratch2.copy_(scratch)
            return []
        runs = {"a_profile_rows": run_a, "b_torch_recipe": run_b, "copy_ceiling": run_copy, "judge_rows": run_judge}
        for _ in range(args.warmup):
            for f in runs.values():
                f()
        same = all(bool(torch.equal(res["a"][k], res["b"][k])) for k in TABLES)
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
        out = {"tool": "profile_bench", "workload": "rows of synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d) at row_len %d; pairs, codes, six tables, "
               "%d cycles, %d score bins; %s" % (fastq_bytes / 2e9, args.pairs, args.seed, L, L, args.qbins, label),
               "triple": label, "rows": n, "rows_bytes": traffic, "reps": args.reps, "summary": summary, "a_equals_b": same}
        for k, v in ms.items():
            s = sorted(v)
            out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
        a_ms = out["a_profile_rows"]["ms_median"]; st = out["a_profile_rows"]["stages_ms"]
        out["a_over_b"] = round(a_ms / out["b_torch_recipe"]["ms_median"], 5)
        out["rows_bytes_per_s_over_hbm_peak"] = round(traffic / (a_ms * 1e-3) / HBM_PEAK, 4)
        out["kernel_bytes_per_s_over_hbm_peak"] = round(traffic / (max(st.get("profile:rows", 0.0), 1e-9) * 1e-3) / HBM_PEAK, 4)
        out["copy_share_of_a"] = round(out["copy_ceiling"]["ms_median"] / max(a_ms, 1e-9), 3)
        out["kernel_over_judge_kernel"] = round(st.get("profile:rows", 0.0) / max(out["judge_rows"]["stages_ms"].get("judge:rows", 0.0), 1e-9), 3)
        print(json.dumps(out), flush=True)
        if not same:
            rc = 1
        del scratch, scratch2
    codec.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
