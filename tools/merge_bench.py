"""rfq_merge_rows beside rfq_select_rows and a copy, on one context, one process.  The rows are tools/adapter_bench.py's (fragments of a pseudo-genome read from
both ends as reads of 150 at row_len 160, codes); --pairs sets the size (default 1.4 M pairs = 2.8 M rows).  The inserts are drawn here, uniform in [100, 290) for
80 % of the pairs and -1 for the rest: the merge takes no decision, so its cost depends on the inserts and not on whether the mates really overlap there.  Before
timing, the first 4096 pairs are checked against the host loop of tests/_merge.py.  Warmed up, alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.merge_pairs(unmerged=False) at the output row_len 304
  (b) repaq_amd.tensors.select_rows keeping every row of the same tensors (the project's yardstick for a byte mover)
  (c) a device-to-device copy of as many bytes as merge:rows reads and writes: 2 * (l1 + l2) + 2 * insert per merged pair (select:rows: 2 * l per row read, 2 * row_len
      written)
One JSON line: ms (median, min, all), the merge:rows and select:rows stages, bytes moved by each, ns per KiB moved of both, their ratio, the copy's share.
    python tools/merge_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_400_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--read", type=int, default=150)
    ap.add_argument("--out-row-len", type=int, default=304)
    ap.add_argument("--check", type=int, default=4096)
    args = ap.parse_args()
    import numpy as np
    import torch
    import _merge as M
    import _rows as W
    from adapter_bench import make_rows
    from repaq_amd import RfqCodec
    from repaq_amd.tensors import merge_pairs, select_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    L = args.row_len
    bases, quals, lens, _ = make_rows(torch, dev, args.pairs, L, args.read, args.seed, 0.003)
    g = torch.Generator(device=dev); g.manual_seed(args.seed + 1)
    insert = torch.randint(100, 290, (args.pairs,), generator=g, device=dev, dtype=torch.int32)
    insert = torch.where(torch.rand((args.pairs,), generator=g, device=dev) < 0.8, insert, torch.full_like(insert, -1))
    t = {"bases": bases, "quals": quals, "lens": lens}
    n = 2 * args.pairs
    # the first pairs against the host loop
    nc = min(args.check, args.pairs)
    head = {k: v[:2 * nc].contiguous() for k, v in t.items()}
    got = merge_pairs(codec, head, insert[:nc].contiguous(), row_len=args.out_row_len, unmerged=False)
    e = M.expected(*(head[k].cpu().numpy() for k in ("bases", "quals", "lens")), None, insert[:nc].cpu().numpy(), True)
    assert got["summary"] == dict(zip(M.FIELDS, e["result"])), (got["summary"], e["result"])
    for k, pad in (("bases", 255), ("quals", 255)):
        assert np.array_equal(got["merged"][k].cpu().numpy(), W.padded(e[k], args.out_row_len, pad)), k
    merged = insert >= 0
    moved_merge = int((2 * (lens.view(-1, 2).sum(1)[merged].sum()) + 2 * insert[merged].sum()).item())
    moved_select = 2 * int(lens.sum().item()) + 2 * n * L                    # (bases and scores: the reads read, whole rows written)
    res = {}

    def run_m():
        res["m"] = merge_pairs(codec, t, insert, row_len=args.out_row_len, unmerged=False)
        return codec.timings()

    def run_s():
        res["s"] = select_rows(codec, t, row_len=L)
        return codec.timings()
    src = torch.empty((moved_merge // 2,), dtype=torch.uint8, device=dev); dst = torch.empty_like(src)

    def run_copy():
        dst.copy_(src)
        return []
    runs = {"a_merge_pairs": run_m, "b_select_rows_all": run_s, "copy_of_the_bytes_merge_rows_moves": run_copy}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    summary = res["m"]["summary"]
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            res.clear()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for name, v in st:
                stages[k][name] = stages[k].get(name, 0.0) + v / args.reps
    out = {"tool": "merge_bench", "workload": "%d pairs of reads of %d at row_len %d (codes), inserts uniform in [100, 290) for 80 %% of the pairs, -1 for the rest, seed %d; "
           "merged rows at row_len %d; select_rows keeps every row at row_len %d" % (args.pairs, args.read, L, args.seed, args.out_row_len, L),
           "rows": n, "reps": args.reps, "checked_pairs": nc, "summary": summary, "bytes_moved_merge_rows": moved_merge, "bytes_moved_select_rows": moved_select}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    mr = out["a_merge_pairs"]["stages_ms"].get("merge:rows", 0.0); sr = out["b_select_rows_all"]["stages_ms"].get("select:rows", 0.0)
    out["merge_rows_ns_per_kib"] = round(mr * 1e6 / (moved_merge / 1024), 3); out["select_rows_ns_per_kib"] = round(sr * 1e6 / (moved_select / 1024), 3)
    out["merge_rows_over_select_rows_per_byte"] = round(out["merge_rows_ns_per_kib"] / max(out["select_rows_ns_per_kib"], 1e-9), 3)
    out["merge_rows_gb_per_s"] = round(moved_merge / max(mr, 1e-9) / 1e6, 1); out["select_rows_gb_per_s"] = round(moved_select / max(sr, 1e-9) / 1e6, 1)
    out["copy_gb_per_s"] = round(moved_merge / out["copy_of_the_bytes_merge_rows_moves"]["ms_median"] / 1e6, 1)
    out["copy_share_of_merge_rows"] = round(out["copy_of_the_bytes_merge_rows_moves"]["ms_median"] / max(mr, 1e-9), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
