"""rfq_kmers_rows under its three formulations against two yardsticks that are not the code under test, on one context, one process (rows: fastq_to_tensors of
synthetic NovaSeq PE150 in two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 1 M reads at row_len 160, base
codes).  Three cases, each into a fresh table of 2 x its distinct values (counted by the torch yardstick first):
  k25_random    k = 25, the rows as generated: almost no value comes twice
  k25_tails     k = 25, 10 % of the rows end in 60 x G, 5 % run into an adapter and A's from a random position on: a few values take a large share of the adds,
                and around them lie the k-mers that share a suffix
  k5            k = 5: every add goes to one of 512 values
Each case under RFQ_KMERS = default (a workgroup combines in LDS), direct (no LDS stage) and general (a wave per row), warmed up, alternating and repeated, timed
with device events around tensors.count_kmers, with its stage time kmers:rows; the table is formatted again before every run, outside the timing.  Beside them:
  screen        rfq_screen_rows on the same rows against an index in device memory (a random reference of 4 M bases): the same k-mer forming plus a probe without
                the add - the cost of counting is the difference
  torch         the k-mers of the code rows packed to canonical int64 values (k shifted slices of the [n, L] rows: the [n, W, k] tensor of a literal unfold does
                not fit), torch.unique(return_counts=True)
The default formulation's table is read back (tensors.kmer_counts) and compared with torch.unique's values and counts, entry by entry.  One JSON line per case: ms
(median, min, max, all) per formulation and yardstick, the spread, the table's size.  No ratio is fixed in advance: exit status 0 when every line was produced and
the tables equal torch's.
    python tools/kmers_bench.py [--pairs N] [--reps K] [--cases k25_random,k25_tails,k5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--cases", type=str, default="k25_random,k25_tails,k5")
    ap.add_argument("--forms", type=str, default="default,direct,general")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch yardstick's timing out (the distinct values are still counted with it, once)")
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, kmer_table, count_kmers, kmer_counts, screen_index, screen_rows
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    L = args.row_len
    t0 = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L, names=False)
    del t1, t2
    n = t0["lens"].numel()
    assert n == 2 * args.pairs and L >= 150
    gen = torch.Generator(device=dev); gen.manual_seed(args.seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code_of = {65: 0, 67: 1, 71: 2, 84: 3}
    adapter = torch.tensor([code_of[c] for c in ADAPTER], dtype=torch.uint8, device=dev)

    def canonical(codes, lens, k):
        """[m, L] codes, [m] lens -> the canonical int64 values of the valid k-mers inside the reads, one flat tensor"""
        W = L - k + 1
        c = codes.to(torch.int64)
        fwd = torch.zeros((c.shape[0], W), dtype=torch.int64, device=dev); rc = torch.zeros_like(fwd); ok = torch.ones_like(fwd, dtype=torch.bool)
        for i in range(k):
            s = c[:, i:i + W]
            fwd = fwd * 4 + (s & 3); rc = rc + ((3 - (s & 3)) << (2 * i)); ok &= s < 4
        ok &= (torch.arange(W, device=dev, dtype=torch.int32)[None, :] + k) <= lens[:, None]
        return torch.minimum(fwd, rc)[ok]

    def torch_counts(t, k):
        step = 1 << 18                                                      # (rows per slice: the int64 intermediates of 2 M rows at once are tens of GB)
        vals = torch.cat([canonical(t["bases"][r0:r0 + step], t["lens"][r0:r0 + step], k) for r0 in range(0, n, step)])
        return torch.unique(vals, return_counts=True)

    ok_all = True
    for case in args.cases.split(","):
        k = 5 if case == "k5" else 25
        t = {key: t0[key].clone() for key in ("bases", "lens")}
        if case == "k25_tails":
            rows = torch.randperm(n, device=dev, generator=gen)
            g_rows = rows[:n // 10]; a_rows = rows[n // 10:n // 10 + n // 20]
            t["bases"][g_rows, 90:150] = 2; t["lens"][g_rows] = 150
            at = torch.randint(60, 110, (a_rows.numel(),), device=dev, generator=gen)
            col = torch.arange(150, device=dev)[None, :]; rel = col - at[:, None]
            tail = torch.where(rel < len(ADAPTER), adapter[rel.clamp(0, len(ADAPTER) - 1)], torch.zeros((), dtype=torch.uint8, device=dev))
            t["bases"][a_rows, :150] = torch.where(rel >= 0, tail, t["bases"][a_rows, :150]); t["lens"][a_rows] = 150
        ev = lambda: torch.cuda.Event(enable_timing=True)
        e0, e1 = ev(), ev()
        torch.cuda.synchronize(); e0.record(); uv, uc = torch_counts(t, k); e1.record(); torch.cuda.synchronize()
        torch_ms = [e0.elapsed_time(e1)]
        distinct, total = int(uv.numel()), int(uc.sum())
        ref_n = 4_000_000
        ix = screen_index(codec, (letters[torch.randint(0, 4, (ref_n,), device=dev, generator=gen)], torch.tensor([0, ref_n], dtype=torch.int64, device=dev)), k=k)
        tab = kmer_table(codec, k=k, slots=2 * distinct)
        res = {}

        def run_form(form):
            def f():
                codec.set_option("RFQ_KMERS", None)
                codec.kmers_init(k=k, slots=2 * distinct, d_table=tab["table"].data_ptr(), table_cap=tab["table"].numel())
                codec.set_option("RFQ_KMERS", None if form == "default" else form)
                torch.cuda.synchronize(); e0.record()
                res[form] = count_kmers(codec, t, tab)
                e1.record(); torch.cuda.synchronize()
                codec.set_option("RFQ_KMERS", None)
                return e0.elapsed_time(e1), dict(codec.timings())
            return f

        def run_screen():
            torch.cuda.synchronize(); e0.record()
            res["screen"] = screen_rows(codec, t, ix)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1), dict(codec.timings())
        runs = {form: run_form(form) for form in args.forms.split(",")}
        runs["screen"] = run_screen
        for _ in range(args.warmup):
            for f in runs.values():
                f()
        # the default formulation's table against torch.unique, entry by entry; every formulation's summary against its counts
        same = True
        for form in args.forms.split(","):
            s = res[form]["summary"]
            same = same and (s["n_kmers"], s["total"], s["added"], s["lost"]) == (distinct, total, total, 0)
        runs[args.forms.split(",")[0]]()
        kc = kmer_counts(codec, tab)
        same = same and bool(torch.equal(kc["values"], uv)) and bool(torch.equal(kc["counts"], uc))
        same = same and bool(torch.equal(res[args.forms.split(",")[0]]["kmers"], res["screen"]["kmers"]))
        top = int(uc.max()) if distinct else 0
        del kc
        ms = {key: [] for key in runs}; stage = {key: [] for key in runs}
        for _ in range(args.reps):
            for key, f in runs.items():
                wall, st = f()
                ms[key].append(wall); stage[key].append(st.get("kmers:rows", st.get("screen:rows", 0.0)))
        if not args.no_torch:
            for _ in range(min(args.reps, 2)):
                del uv, uc
                torch.cuda.synchronize(); e0.record(); uv, uc = torch_counts(t, k); e1.record(); torch.cuda.synchronize()
                torch_ms.append(e0.elapsed_time(e1))
        out = {"tool": "kmers_bench", "case": case, "k": k, "rows": n, "row_len": L, "adds": total, "distinct": distinct, "largest_count": top, "slots": tab["slots"],
               "table_bytes": int(tab["table"].numel()), "reps": args.reps, "table_equals_torch_unique": same}

        def stat(v):
            s = sorted(v)
            return {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_max": round(s[-1], 3), "ms_all": [round(x, 3) for x in v]}
        for key in runs:
            out[key] = dict(stat(ms[key]), stage=stat(stage[key]))
        out["torch_unique"] = stat(torch_ms)
        print(json.dumps(out), flush=True)
        ok_all = ok_all and same
        del t, tab, ix, uv, uc
        torch.cuda.empty_cache()
    codec.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
