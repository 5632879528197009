"""rfq_screen_rows against the torch recipe for the same hits tensor, on one context, one process (configs[2]-shaped rows: fastq_to_tensors of synthetic NovaSeq
PE150 in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160, base codes).  A share of
the pairs (0 %, 1 %, 50 %) is planted from the reference: R1 a window of it, R2 the reverse complement of a window.  Two indexes, k = 25:
  lds     a random reference of 5,386 bases (PhiX's size): S = 16384 slots, the table in LDS
  device  a random reference of 4 M bases: S = 8 M slots, the table in device memory
Warmed up, alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.screen_rows: the output tensors and the call (keep, hits, kmers and the summary), with its stage time screen:rows
  (b) the same hits tensor in torch: the windows of the code rows (an unfold, written as k shifted slices of the [n, L] rows - the [n, W, k] int64 tensor of a
      literal unfold does not fit) packed to int64 forward and reverse-complement values, canonical by torch.minimum, torch.isin against the sorted set, summed under
      the validity mask - checked equal to (a) once before timing
Beside them, not gated: a device-to-device copy of the bytes (a) reads from the rows (its ceiling).
One JSON line per index and share: ms (median, min, all), the stage, a over b, the copy over a, bytes of rows / time of (a) against the HBM peak DESIGN.md §5 uses
(8 TB/s), and the index build's time.  No ratio is fixed in advance: exit status 0 when every line was produced and (a) equals (b).
    python tools/screen_bench.py [--pairs N] [--reps K]"""
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--k", type=int, default=25)
    ap.add_argument("--shares", type=str, default="0,1,50")
    ap.add_argument("--refs", type=str, default="lds:5386,device:4000000")
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, screen_index, screen_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    fastq_bytes = t1.numel() + t2.numel()
    del a1, a2
    L, k = args.row_len, args.k
    t0 = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L, names=False)
    del t1, t2
    n = t0["lens"].numel(); U = n // 2
    assert n == 2 * args.pairs and L >= 150
    gen = torch.Generator(device=dev); gen.manual_seed(args.seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    W = L - k + 1
    pos = torch.arange(W, device=dev, dtype=torch.int32)

    def packed(codes):
        """[m, L] codes -> (canonical int64 [m, W], all-ACGT mask [m, W]) of the k-mers at every window start"""
        c = codes.to(torch.int64)
        fwd = torch.zeros((c.shape[0], W), dtype=torch.int64, device=dev); rc = torch.zeros_like(fwd); ok = torch.ones_like(fwd, dtype=torch.bool)
        for i in range(k):
            s = c[:, i:i + W]
            fwd = fwd * 4 + (s & 3); rc = rc + ((3 - (s & 3)) << (2 * i)); ok &= s < 4
        return torch.minimum(fwd, rc), ok
    ok_all = True
    for spec in args.refs.split(","):
        label, ref_n = spec.split(":"); ref_n = int(ref_n)
        ref = torch.randint(0, 4, (ref_n,), device=dev, generator=gen, dtype=torch.uint8)
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        ix = screen_index(codec, (letters[ref.long()], torch.tensor([0, ref_n], dtype=torch.int64, device=dev)), k=k)
        e1.record(); torch.cuda.synchronize()
        build_ms = e0.elapsed_time(e1)
        # the sorted set of the recipe: the reference's own windows (row by row of a [1, ref_n] "row" would need W = ref_n: in slices of L with k - 1 overlap)
        starts = torch.arange(0, ref_n - k + 1, W, device=dev)
        idx = (starts[:, None] + torch.arange(L, device=dev)[None, :]).clamp_(max=ref_n - 1)
        rows_ref = torch.where(starts[:, None] + torch.arange(L, device=dev)[None, :] < ref_n, ref[idx], torch.full((), 4, dtype=torch.uint8, device=dev))
        cv, okv = packed(rows_ref)
        the_set = torch.unique(cv[okv])
        assert the_set.numel() == ix["n_kmers"], (the_set.numel(), ix["n_kmers"])
        del rows_ref, cv, okv, idx
        for share in (int(x) for x in args.shares.split(",")):
            t = {key: t0[key].clone() for key in ("bases", "lens")}
            n_pl = U * share // 100
            if n_pl:
                units = torch.randperm(U, device=dev, generator=gen)[:n_pl]
                j1 = torch.randint(0, ref_n - 150, (n_pl,), device=dev, generator=gen); j2 = torch.randint(0, ref_n - 150, (n_pl,), device=dev, generator=gen)
                w = torch.arange(150, device=dev)
                bv = t["bases"].view(U, 2, L); lv = t["lens"].view(U, 2)
                bv[units, 0, :150] = ref[j1[:, None] + w[None, :]]
                bv[units, 1, :150] = 3 - ref[j2[:, None] + w[None, :]].flip(1)
                lv[units] = 150
            res = {}

            def run_a():
                res["a"] = screen_rows(codec, t, ix, pairs=True)
                return codec.timings()

            def run_b():
                hits = torch.empty((n,), dtype=torch.int32, device=dev)
                step = 1 << 18                                              # (rows per slice: the int64 intermediates of 2 M rows at once are tens of GB)
                for r0 in range(0, n, step):
                    cv, okv = packed(t["bases"][r0:r0 + step])
                    okv &= (pos[None, :] + k) <= t["lens"][r0:r0 + step, None]
                    hits[r0:r0 + step] = (torch.isin(cv, the_set, assume_unique=False) & okv).sum(1)
                res["b"] = {"hits": hits}
                return []

            traffic = n * L + 4 * n                                          # (a) reads the base rows and a length per row once
            scratch = torch.empty(traffic, dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

            def run_copy():
                scratch2.copy_(scratch)
                return []
            runs = {"a_screen_rows": run_a, "b_torch_recipe": run_b, "copy_ceiling": run_copy}
            for _ in range(args.warmup):
                for f in runs.values():
                    f()
            same = bool(torch.equal(res["a"]["hits"], res["b"]["hits"]))
            summary = res["a"]["summary"]
            ms = {key: [] for key in runs}; stages = {key: {} for key in runs}
            for _ in range(args.reps):
                for key, f in runs.items():
                    res.clear()
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
                    ms[key].append(e0.elapsed_time(e1))
                    for name, v in st:
                        stages[key][name] = stages[key].get(name, 0.0) + v / args.reps
            out = {"tool": "screen_bench", "workload": "rows of synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d) at row_len %d, codes, %d %% of the pairs "
                   "planted from a random reference of %d bases; pairs, k %d, min_hits 1" % (fastq_bytes / 2e9, args.pairs, args.seed, L, share, ref_n, k),
                   "index": label, "ref_bases": ref_n, "slots": ix["slots"], "n_kmers": ix["n_kmers"], "placement": "lds" if ix["slots"] <= 16384 else "device memory",
                   "build_ms": round(build_ms, 3), "planted_pct": share, "rows": n, "units": U, "rows_bytes": traffic, "reps": args.reps, "summary": summary, "a_equals_b": same}
            for key, v in ms.items():
                s = sorted(v)
                out[key] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[key].items()}}
            a_ms = out["a_screen_rows"]["ms_median"]; st = out["a_screen_rows"]["stages_ms"]
            out["a_over_b"] = round(a_ms / out["b_torch_recipe"]["ms_median"], 5)
            out["copy_over_a"] = round(out["copy_ceiling"]["ms_median"] / max(a_ms, 1e-9), 4)
            out["rows_bytes_per_s_over_hbm_peak"] = round(traffic / (a_ms * 1e-3) / HBM_PEAK, 4)
            out["kernel_bytes_per_s_over_hbm_peak"] = round(traffic / (max(st.get("screen:rows", 0.0), 1e-9) * 1e-3) / HBM_PEAK, 4)
            print(json.dumps(out), flush=True)
            ok_all = ok_all and same
            del t, scratch, scratch2
        del the_set, ix
    codec.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
