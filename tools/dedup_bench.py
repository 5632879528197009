"""rfq_dedup_rows against the torch recipe for the same keep mask, on one context, one process (configs[2]-shaped rows: fastq_to_tensors of synthetic NovaSeq PE150
in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160).  A share of the pairs is
planted as copies of other pairs of the batch, both mates: duplication rates 0 %, 10 % and 50 %.  Pairs, RFQ_DEDUP_FIRST, the whole read as the key.  Warmed up,
alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.dedup_rows: the output tensors and the call (keep, dup_of, count and the summary), with its stage times dedup:key / :claim / :resolve
  (b) the same keep mask in torch: the bases under a length mask, both mates and both lengths side by side as ONE row per pair, torch.unique(dim=0,
      return_inverse=True) - a lexicographic sort of 322-byte keys - and a scatter-min of the unit index over the inverse - checked equal to (a) once before timing
Beside them, not gated: a device-to-device copy of the bytes (a) reads from the rows (its ceiling).
One JSON line per duplication rate: ms (median, min, all), the stages, a over b, bytes of rows / time of (a) against the HBM peak DESIGN.md §5 uses (8 TB/s), and
the claim kernel's atomics per unit (counted from the result, not measured: one compare-and-swap per class, one max and one add per candidate).  No ratio is fixed
in advance: exit status 0 when every line was produced and (a) equals (b).
    python tools/dedup_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--rates", type=str, default="0,10,50")
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, dedup_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    fastq_bytes = t1.numel() + t2.numel()
    del a1, a2
    L = args.row_len
    t0 = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L, names=False)
    del t1, t2
    n = t0["lens"].numel(); U = n // 2
    assert n == 2 * args.pairs and L <= 255
    gen = torch.Generator(device=dev); gen.manual_seed(args.seed)
    unit = torch.arange(U, device=dev)
    for rate in (int(x) for x in args.rates.split(",")):
        # `rate` % of the pairs become copies of pairs that stay as they are
        perm = torch.randperm(U, device=dev, generator=gen)
        n_dup = U * rate // 100
        dst, keepers = perm[:n_dup], perm[n_dup:]
        src = keepers[torch.randint(0, keepers.numel(), (n_dup,), device=dev, generator=gen)] if n_dup else dst
        t = {k: t0[k].clone() for k in ("bases", "quals", "lens")}
        for k in ("bases", "lens"):
            v = t[k].view(U, 2, -1) if k == "bases" else t[k].view(U, 2)
            v[dst] = v[src]
        res = {}

        def run_a():
            res["a"] = dedup_rows(codec, t, pairs=True)
            return codec.timings()

        def run_b():
            bases, lens = t["bases"], t["lens"]
            inside = torch.arange(L, device=dev, dtype=torch.int32)[None, :] < lens[:, None]
            key = torch.cat([torch.where(inside, bases, 0).view(U, 2 * L), lens.to(torch.uint8).view(U, 2)], dim=1)       # (a length fits a byte: L <= 255)
            _, inv = torch.unique(key, dim=0, return_inverse=True)
            first = torch.full((int(inv.max()) + 1,), U, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, unit, "amin")
            res["b"] = {"keep": (first[inv] == unit).to(torch.uint8).repeat_interleave(2)}
            return []

        traffic = n * L + 4 * n                                              # (a) reads the base rows and a length per row once in the key kernel
        scratch = torch.empty(traffic, dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

        def run_copy():
            scratch2.copy_(scratch)
            return []
        runs = {"a_dedup_rows": run_a, "b_torch_recipe": run_b, "copy_ceiling": run_copy}
        for _ in range(args.warmup):
            for f in runs.values():
                f()
        same = bool(torch.equal(res["a"]["keep"], res["b"]["keep"]))
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
        out = {"tool": "dedup_bench", "workload": "rows of synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d) at row_len %d, %d %% of the pairs planted as "
               "copies; pairs, FIRST, whole reads" % (fastq_bytes / 2e9, args.pairs, args.seed, L, rate),
               "dup_rate_pct": rate, "rows": n, "units": U, "rows_bytes": traffic, "reps": args.reps, "summary": summary, "a_equals_b": same}
        for k, v in ms.items():
            s = sorted(v)
            out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
        a_ms = out["a_dedup_rows"]["ms_median"]; st = out["a_dedup_rows"]["stages_ms"]
        out["a_over_b"] = round(a_ms / out["b_torch_recipe"]["ms_median"], 5)
        out["rows_bytes_per_s_over_hbm_peak"] = round(traffic / (a_ms * 1e-3) / HBM_PEAK, 4)
        out["key_kernel_bytes_per_s_over_hbm_peak"] = round(traffic / (max(st.get("dedup:key", 0.0), 1e-9) * 1e-3) / HBM_PEAK, 4)
        out["copy_share_of_a"] = round(out["copy_ceiling"]["ms_median"] / max(a_ms, 1e-9), 3)
        out["claim_share_of_stages"] = round(st.get("dedup:claim", 0.0) / max(sum(st.values()), 1e-9), 3)
        out["claim_atomics_per_unit"] = round((summary["n_classes"] + 2 * summary["n_candidates"]) / max(U, 1), 3)
        print(json.dumps(out), flush=True)
        if not same:
            codec.close()
            return 1
        del t, scratch, scratch2
    codec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
