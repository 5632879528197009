"""rfq_group_rows against the two things it stands between, on one context, one process (rows: fastq_to_tensors of synthetic NovaSeq PE150 in two files, fqgen
profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160, base codes).  The case is tools/demux_bench.py's
a_96x8: 96 barcodes of 8 bases planted over the front of read 1 with 1 % of their bases replaced, demux_rows with max_mm = 1, min_delta = 1 gives the sample per
pair and the start behind the barcode: 96 samples and the unassigned, 97 bins.  Alternating, warmed up, repeated, timed with device events:
  group       tensors.group_rows(bin=sample, start=start, pairs=True) + group_parts: one pass over the rows, ONE read-back for the parts
  split_rows  tensors.split_rows with the same inputs: one select_rows pass per bin that holds a row - what grouping replaces
  select_all  tensors.select_rows with every row kept and the same start: the same bytes moved once in INPUT order - the floor grouping can approach
The stage times of group_rows' writing call come from rfq_last_timings (group:judge, group:rank, group:tables, group:rows, group:names), and those of select_all's
(select:judge .. select:names) beside them.  Every part of group
is compared with split_rows' (lens, names, offsets, the rows up to each length).  One JSON line: ms (median, min, max, all) per yardstick, the stages, group over
split_rows and over select_all, group:rank's share of the stages.  No time or ratio is fixed in advance: exit status 0 when the line was produced and the parts
are equal.
    python tools/group_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
STAGES = ("group:judge", "group:rank", "group:tables", "group:rows", "group:names")
FLOOR_STAGES = ("select:judge", "select:tables", "select:rows", "select:names")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--row-len", type=int, default=160)
    args = ap.parse_args()
    import numpy as np
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, demux_rows, split_rows, select_rows, group_rows, group_parts
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    L = args.row_len
    t = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L)
    del t1, t2
    n = t["lens"].numel(); U = n // 2
    assert n == 2 * args.pairs and L >= 150
    gen = torch.Generator(device=dev); gen.manual_seed(args.seed)
    rng = np.random.default_rng(args.seed)
    n1, ln = 96, 8
    seen = set(); set1 = []
    while len(set1) < n1:
        c = bytes(rng.integers(0, 4, ln).astype(np.uint8))
        if c not in seen:
            seen.add(c); set1.append(c)
    bc1 = torch.tensor(np.frombuffer(b"".join(set1), np.uint8).reshape(n1, ln), device=dev)
    who = torch.randint(0, n1, (U,), device=dev, generator=gen)
    codes = bc1[who]
    err = torch.rand(codes.shape, device=dev, generator=gen) < 0.01
    other = (codes + 1 + torch.randint(0, 3, codes.shape, device=dev, generator=gen, dtype=torch.uint8)) & 3
    t["bases"][torch.arange(0, n, 2, device=dev), :ln] = torch.where(err, other, codes)
    dm = demux_rows(codec, t, [bytes(b"ACGT"[c] for c in b) for b in set1], pairs=True, max_mm=1, min_delta=1)
    sample, start = dm["sample"], dm["start"]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    e0, e1 = ev(), ev()
    res = {}

    def run_group():
        torch.cuda.synchronize(); e0.record()
        g = group_rows(codec, t, sample, n1, start=start, pairs=True)
        st = dict(codec.timings())
        parts = group_parts(g)
        e1.record(); torch.cuda.synchronize()
        res["group"] = (g, parts)
        return e0.elapsed_time(e1), st

    def run_split():
        torch.cuda.synchronize(); e0.record()
        parts = split_rows(codec, t, sample, n1, start=start, pairs=True)
        e1.record(); torch.cuda.synchronize()
        res["split_rows"] = parts
        return e0.elapsed_time(e1), {}

    def run_select():
        torch.cuda.synchronize(); e0.record()
        s = select_rows(codec, t, start=start, pairs=True)
        st = dict(codec.timings())
        e1.record(); torch.cuda.synchronize()
        res["select_all"] = int(s["lens"].numel())
        return e0.elapsed_time(e1), st
    runs = {"group": run_group, "split_rows": run_split, "select_all": run_select}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    # every part of group equals split_rows' (split_rows pads a bin to its own longest row)
    g, parts = res["group"]; split = res["split_rows"]
    same = len(parts) == len(split) == n1 + 1
    for p, s in zip(parts, split):
        if p is None or s is None:
            same = same and p is None and s is None
            continue
        ok = torch.equal(p["lens"], s["lens"]) and torch.equal(p["names"], s["names"]) and torch.equal(p["name_off"], s["name_off"])
        ls = s["bases"].shape[1]
        inside = torch.arange(ls, device=dev)[None, :] < s["lens"][:, None]
        for key in ("bases", "quals"):
            ok = ok and torch.equal(torch.where(inside, p[key][:, :ls], torch.zeros_like(s[key])), torch.where(inside, s[key], torch.zeros_like(s[key])))
        same = same and bool(ok)
    rows_moved = int(g["lens"].numel())
    bins_used = sum(1 for p in parts if p is not None)
    del g, parts, split
    res.clear(); torch.cuda.empty_cache()
    ms = {key: [] for key in runs}; stages = {k: [] for k in STAGES + FLOOR_STAGES}
    for _ in range(max(args.reps, 2)):
        for key, f in runs.items():
            wall, st = f()
            ms[key].append(wall)
            for k in STAGES + FLOOR_STAGES:
                if k in st:
                    stages[k].append(st[k])
        res.clear()

    def stat(v):
        s = sorted(v)
        return {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_max": round(s[-1], 3), "ms_all": [round(x, 3) for x in v]}
    out = {"tool": "group_bench", "rows": n, "row_len": L, "bins": n1 + 1, "bins_used": bins_used, "rows_moved": rows_moved, "reps": max(args.reps, 2),
           "parts_equal_split_rows": same}
    for key in runs:
        out[key] = stat(ms[key])
    out["stages"] = {k: stat(stages[k])["ms_median"] for k in STAGES if stages[k]}
    out["select_all_stages"] = {k: stat(stages[k])["ms_median"] for k in FLOOR_STAGES if stages[k]}
    total = sum(out["stages"].values())
    out["rank_share_of_stages"] = round(out["stages"].get("group:rank", 0.0) / total, 4) if total else None
    out["group_over_split_rows"] = round(out["group"]["ms_median"] / out["split_rows"]["ms_median"], 4)
    out["group_over_select_all"] = round(out["group"]["ms_median"] / out["select_all"]["ms_median"], 4)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
