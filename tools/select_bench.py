"""rfq_select_rows against the torch recipe it replaces, on one context, one process (configs[2]-shaped rows: fastq_to_tensors of synthetic NovaSeq PE150 in
two files, fqgen profile 1, seed 3 - bench.py's generator path; --pairs sets the size, the default is 2 x 11.2 M reads at row_len 160).  A seeded selection keeps
about 80 % of the pairs and trims 0..30 bases off each end of every read.  Warmed up, alternating and repeated, timed with device events:
  (a) repaq_amd.tensors.select_rows: the size query, the output tensors and the call (rows, lengths, names and offsets, row_len 160)
  (b) the same tensors without it: the module docstring's earlier recipe (boolean-index copies of the rows, repeat_interleave + arange + cumsum to re-pack the name
      blob) extended with a torch.gather over an [n, L] index for the trim - without the trim it would do less work than (a)
Beside them, not gated: rfq_select_rows alone into tensors allocated up front (a_call_only: its stages are those of rfq_last_timings), and a device-to-device copy
of the bytes (a) reads and writes (its ceiling).
One JSON line: ms (median, min, all), the stages, a over b, the copy's share of (a).  Exit status 0 when the median of (a) is below the median of (b).
    python tools/select_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11_200_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import fastq_to_tensors, select_rows
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
    g = torch.Generator(device=dev); g.manual_seed(args.seed)
    keep = (torch.rand(args.pairs, device=dev, generator=g) < 0.8).repeat_interleave(2)
    head = torch.randint(0, 31, (n,), device=dev, generator=g, dtype=torch.int32); tail = torch.randint(0, 31, (n,), device=dev, generator=g, dtype=torch.int32)
    start = torch.minimum(head, t["lens"] - 1).contiguous(); length = torch.clamp(t["lens"] - start - tail, min=1).contiguous()
    res = {}

    def run_a():
        res["a"] = select_rows(codec, t, keep=keep, start=start, length=length, pairs=True, row_len=L)
        return codec.timings()

    def run_b():
        bases, quals, off = t["bases"], t["quals"], t["name_off"]
        ln = off[1:] - off[:-1]
        new_off = torch.cat([off[:1], ln[keep].cumsum(0)])
        src = torch.repeat_interleave(off[:-1][keep] - new_off[:-1], ln[keep]) + torch.arange(int(new_off[-1]), device=dev)
        names = t["names"][src]
        ks, kl = start[keep].long(), length[keep]
        col = torch.arange(L, device=dev)
        idx = (ks[:, None] + col[None, :]).clamp_(max=bases.shape[1] - 1)
        pad = col[None, :] >= kl[:, None]
        ob = torch.gather(bases[keep], 1, idx).masked_fill_(pad, 255); oq = torch.gather(quals[keep], 1, idx).masked_fill_(pad, 255)
        res["b"] = {"bases": ob, "quals": oq, "lens": kl, "names": names, "name_off": new_off}
        return []

    q = codec.select_rows(n, L, t["bases"].data_ptr(), t["quals"].data_ptr(), t["lens"].data_ptr(), t["names"].data_ptr(), t["names"].numel(), t["name_off"].data_ptr(),
                          d_keep=keep.data_ptr(), d_start=start.data_ptr(), d_len=length.data_ptr(), pairs=True)
    m, nl, nb = int(q.n_rows), int(q.names_len), int(q.n_bases)
    ob = torch.empty((m, L), dtype=torch.uint8, device=dev); oq = torch.empty_like(ob); ol = torch.empty((m,), dtype=torch.int32, device=dev)
    on = torch.empty((nl,), dtype=torch.uint8, device=dev); oo = torch.empty((m + 1,), dtype=torch.int64, device=dev)

    def run_call():
        codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        try:
            codec.select_rows(n, L, t["bases"].data_ptr(), t["quals"].data_ptr(), t["lens"].data_ptr(), t["names"].data_ptr(), t["names"].numel(), t["name_off"].data_ptr(),
                              d_keep=keep.data_ptr(), d_start=start.data_ptr(), d_len=length.data_ptr(), pairs=True, row_len=L, out_bases=ob.data_ptr(), bases_cap=m * L,
                              out_quals=oq.data_ptr(), quals_cap=m * L, out_lens=ol.data_ptr(), lens_cap=m, out_names=on.data_ptr(), names_cap=nl,
                              out_name_off=oo.data_ptr(), off_cap=m + 1)
            return codec.timings()
        finally:
            codec.set_stream(None)

    # the ceiling: a copy of k bytes reads k and writes k.  (a) reads the kept windows of both row arrays, the kept names, and per input row a length, a window, a
    # mask byte and a name offset; it writes two row arrays at row_len, the names, a length and an offset per kept row
    traffic = (2 * nb + nl + n * (4 + 4 + 4 + 1 + 8)) + (2 * m * L + nl + m * (4 + 8))
    scratch = torch.empty(traffic // 2, dtype=torch.uint8, device=dev); scratch2 = torch.empty_like(scratch)

    def run_copy():
        scratch2.copy_(scratch)
        return []
    runs = {"a_select_rows": run_a, "b_torch_recipe": run_b, "a_call_only": run_call, "copy_ceiling": run_copy}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    for k in ("bases", "quals", "lens", "names", "name_off"):                 # the two sides make the same tensors
        assert torch.equal(res["a"][k], res["b"][k]), k
    assert torch.equal(ob, res["b"]["bases"]) and torch.equal(on, res["b"]["names"])
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            res.clear()
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for name, v in st:
                stages[k][name] = stages[k].get(name, 0.0) + v / args.reps
    out = {"tool": "select_bench", "workload": "rows of synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d) at row_len %d; ~80 %% of the pairs kept, "
           "0..30 bases trimmed off each end" % (fastq_bytes / 2e9, args.pairs, args.seed, L),
           "rows_in": n, "rows_out": m, "bases_out": nb, "name_bytes_out": nl, "traffic_bytes": traffic, "reps": args.reps,
           "dropped": {"mask": int(q.dropped_mask), "short": int(q.dropped_short), "mate": int(q.dropped_mate)}}
    for k, v in ms.items():
        s = sorted(v)
        out[k] = {"ms_median": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_all": [round(x, 3) for x in v], "stages_ms": {a: round(b, 3) for a, b in stages[k].items()}}
    out["a_over_b"] = round(out["a_select_rows"]["ms_median"] / out["b_torch_recipe"]["ms_median"], 4)
    out["copy_share_of_a"] = round(out["copy_ceiling"]["ms_median"] / max(out["a_select_rows"]["ms_median"], 1e-9), 3)
    out["copy_share_of_call"] = round(out["copy_ceiling"]["ms_median"] / max(out["a_call_only"]["ms_median"], 1e-9), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0 if out["a_select_rows"]["ms_median"] < out["b_torch_recipe"]["ms_median"] else 1


if __name__ == "__main__":
    sys.exit(main())
