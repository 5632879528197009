"""rfq_demux_rows under its two formulations against a torch formulation of the same rule, on one context, one process (rows: fastq_to_tensors of synthetic NovaSeq
PE150 in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160, base codes).  The
barcodes are random and distinct; every pair gets the barcode(s) of a random sample written over the front of its read(s), then 1 % of the barcode bases are
replaced by another base; max_mm = 1, min_delta = 1.  Three cases:
  a_96x8        96 barcodes of 8 bases, one set (read 1)
  b_384x384x10  384 + 384 barcodes of 10 bases with a unique-dual sheet (sample s = the pair (s, s)); 1 % of the pairs get the R2 barcode of another sample
  c_4096x16     4096 barcodes of 16 bases, one set
Each case under RFQ_DEMUX = default (the sets in LDS, a lane per unit) and general (byte by byte against device memory), warmed up, alternating and repeated, timed
with device events around tensors.demux_rows, with its stage time demux:rows (rfq_last_timings).  Beside them:
  torch         the same rule in torch: the window against the set as a [rows, barcodes, len] compare in slices of rows, min / second min, the sheet as a dense table
  split_rows    case a only: tensors.split_rows(start=...) - one select_rows pass per sample, 96 + 1 passes
Every output of the default formulation (sample, why, best, dist, keep, start, counts) is compared with torch's, and general's bytes with default's.  One JSON line
per case: ms (median, min, max, all) per formulation and yardstick.  No time or ratio is fixed in advance: exit status 0 when every line was produced and the
outputs equal torch's.
    python tools/demux_bench.py [--pairs N] [--reps K] [--cases a_96x8,b_384x384x10,c_4096x16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = {"a_96x8": (96, 0, 8), "b_384x384x10": (384, 384, 10), "c_4096x16": (4096, 0, 16)}
NONE, AMBIG, SHORT, COMBO = 1, 2, 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--cases", type=str, default=",".join(CASES))
    ap.add_argument("--no-split", action="store_true", help="leave split_rows out of case a")
    args = ap.parse_args()
    import numpy as np
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, demux_rows, split_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    L = args.row_len
    t0 = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L)
    del t1, t2
    n = t0["lens"].numel(); U = n // 2
    assert n == 2 * args.pairs and L >= 150
    gen = torch.Generator(device=dev); gen.manual_seed(args.seed)
    rng = np.random.default_rng(args.seed)
    max_mm, min_delta = 1, 1

    def make_set(nb, ln):
        seen = set(); out = []
        while len(out) < nb:
            c = bytes(rng.integers(0, 4, ln).astype(np.uint8))
            if c not in seen:
                seen.add(c); out.append(c)
        return out

    def plant(bases, rows, codes, ln):
        """the barcodes' codes ([rows, ln]) over the front of the given rows, 1 % of the bases replaced by another one"""
        err = torch.rand(codes.shape, device=dev, generator=gen) < 0.01
        other = (codes + 1 + torch.randint(0, 3, codes.shape, device=dev, generator=gen, dtype=torch.uint8)) & 3
        bases[rows, :ln] = torch.where(err, other, codes)

    def torch_row(bases, lens, bc, ln):
        """(best, d1, why) per row of the window [0, ln) against bc ([nb, ln] codes), in slices of rows"""
        nb = bc.shape[0]; idx = torch.arange(nb, device=dev, dtype=torch.int32)
        best = torch.empty((bases.shape[0],), dtype=torch.int32, device=dev); d1 = torch.empty_like(best); d2 = torch.empty_like(best)
        step = max(1, (1 << 28) // (nb * ln))
        for r0 in range(0, bases.shape[0], step):
            w = bases[r0:r0 + step, :ln]
            d = ((w[:, None, :] != bc[None, :, :]) | (w[:, None, :] > 3)).sum(dim=2, dtype=torch.int32)
            m = d.min(dim=1).values
            b = torch.where(d == m[:, None], idx[None, :], nb).min(dim=1).values
            d.scatter_(1, b[:, None].to(torch.int64), ln + 1)
            best[r0:r0 + step] = b; d1[r0:r0 + step] = m; d2[r0:r0 + step] = d.min(dim=1).values
        short = lens < ln
        none = ~short & (d1 > max_mm); ambig = ~short & ~none & (d2 - d1 < min_delta)
        why = (short.to(torch.uint8) * SHORT + none.to(torch.uint8) * NONE + ambig.to(torch.uint8) * AMBIG).to(torch.uint8)
        return best.masked_fill(short, -1), d1.masked_fill(short, 255).to(torch.uint8), why

    def torch_demux(t, bc1, bc2, table, ln, n_samples):
        bases, lens = t["bases"], t["lens"]
        b1, x1, w1 = torch_row(bases[0::2], lens[0::2], bc1, ln)
        best = torch.full((n,), -1, dtype=torch.int32, device=dev); dist = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        best[0::2] = b1; dist[0::2] = x1
        why = w1
        if bc2 is not None:
            b2, x2, w2 = torch_row(bases[1::2], lens[1::2], bc2, ln)
            best[1::2] = b2; dist[1::2] = x2; why = w1 | w2
            ok = why == 0
            s = table[b1.clamp(min=0).to(torch.int64), b2.clamp(min=0).to(torch.int64)]
            why = why.masked_fill(ok & (s < 0), COMBO)
            sample = s.masked_fill(why != 0, -1).to(torch.int32)
        else:
            sample = b1.masked_fill(why != 0, -1)
        ok = why == 0
        keep = ok.repeat_interleave(2).to(torch.uint8)
        start = torch.zeros((n,), dtype=torch.int32, device=dev)
        start[0::2] = lens[0::2].clamp(max=ln).masked_fill(~ok, 0)
        if bc2 is not None:
            start[1::2] = lens[1::2].clamp(max=ln).masked_fill(~ok, 0)
        counts = torch.bincount(sample.to(torch.int64).masked_fill(~ok, n_samples), minlength=n_samples + 1)
        return {"sample": sample, "why": why, "best": best, "dist": dist, "keep": keep, "start": start, "counts": counts}

    ok_all = True
    for case in args.cases.split(","):
        n1, n2, ln = CASES[case]
        set1 = make_set(n1, ln); set2 = make_set(n2, ln) if n2 else None
        sheet = [(s, s) for s in range(n1)] if n2 else None
        n_samples = n1
        bc1 = torch.tensor(np.frombuffer(b"".join(set1), np.uint8).reshape(n1, ln), device=dev)
        bc2 = torch.tensor(np.frombuffer(b"".join(set2), np.uint8).reshape(n2, ln), device=dev) if n2 else None
        table = None
        if n2:
            table = torch.full((n1, n2), -1, dtype=torch.int32, device=dev); table[torch.arange(n1, device=dev), torch.arange(n2, device=dev)] = torch.arange(n1, dtype=torch.int32, device=dev)
        asc = lambda s: [bytes(b"ACGT"[c] for c in b) for b in s]
        t = dict(t0, bases=t0["bases"].clone())
        who = torch.randint(0, n1, (U,), device=dev, generator=gen)
        plant(t["bases"], torch.arange(0, n, 2, device=dev), bc1[who], ln)
        if n2:
            hop = torch.rand((U,), device=dev, generator=gen) < 0.01
            who2 = torch.where(hop, torch.randint(0, n2, (U,), device=dev, generator=gen), who)
            plant(t["bases"], torch.arange(1, n, 2, device=dev), bc2[who2], ln)
        kw = dict(barcodes1=asc(set1), barcodes2=asc(set2) if n2 else None, sheet=sheet, pairs=True, max_mm=max_mm, min_delta=min_delta)
        ev = lambda: torch.cuda.Event(enable_timing=True)
        e0, e1 = ev(), ev()
        res = {}

        def run_form(form):
            def f():
                codec.set_option("RFQ_DEMUX", None if form == "default" else form)
                torch.cuda.synchronize(); e0.record()
                res[form] = demux_rows(codec, t, **kw)
                e1.record(); torch.cuda.synchronize()
                codec.set_option("RFQ_DEMUX", None)
                return e0.elapsed_time(e1), dict(codec.timings()).get("demux:rows", 0.0)
            return f

        def run_torch():
            torch.cuda.synchronize(); e0.record()
            res["torch"] = torch_demux(t, bc1, bc2, table, ln, n_samples)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1), 0.0

        def run_split():
            dm = res["default"]
            torch.cuda.synchronize(); e0.record()
            parts = split_rows(codec, t, dm["sample"], n_samples, start=dm["start"], pairs=True)
            e1.record(); torch.cuda.synchronize()
            res["split_rows"] = (sum(1 for p in parts if p is not None), sum(int(p["lens"].numel()) for p in parts if p is not None))
            del parts
            return e0.elapsed_time(e1), 0.0
        runs = {"default": run_form("default"), "general": run_form("general"), "torch": run_torch}
        if case == "a_96x8" and not args.no_split:
            runs["split_rows"] = run_split
        for _ in range(args.warmup):
            for f in runs.values():
                f()
        keys = ("sample", "why", "best", "dist", "keep", "start", "counts")
        same = all(bool(torch.equal(res["default"][k].to(torch.int64), res["torch"][k].to(torch.int64))) for k in keys)
        same_forms = all(bool(torch.equal(res["default"][k], res["general"][k])) for k in keys) and res["default"]["summary"] == res["general"]["summary"]
        summary = res["default"]["summary"]
        ms = {key: [] for key in runs}; stage = {key: [] for key in runs}
        for _ in range(args.reps):
            for key, f in runs.items():
                if key == "torch" and len(ms[key]) >= 2:
                    continue
                wall, st = f()
                ms[key].append(wall); stage[key].append(st)
        out = {"tool": "demux_bench", "case": case, "rows": n, "row_len": L, "n1": n1, "n2": n2, "len": ln, "max_mm": max_mm, "min_delta": min_delta, "reps": args.reps,
               "summary": summary, "outputs_equal_torch": same, "general_equals_default": same_forms}

        def stat(v):
            s = sorted(v)
            return {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_max": round(s[-1], 3), "ms_all": [round(x, 3) for x in v]}
        for key in runs:
            out[key] = stat(ms[key])
            if key in ("default", "general"):
                out[key]["stage"] = stat(stage[key])
        if "split_rows" in res:
            out["split_rows"]["passes"], out["split_rows"]["rows_moved"] = res["split_rows"]
        print(json.dumps(out), flush=True)
        ok_all = ok_all and same and same_forms
        del t, res
        torch.cuda.empty_cache()
    codec.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
