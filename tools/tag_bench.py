"""rfq_select_rows with a tag against the plain call on the same rows and windows, on one context, one process (after tools/select_bench.py: fastq_to_tensors of
synthetic NovaSeq PE150 in two files, fqgen profile 1 - Illumina names of about 60 bytes; --pairs sets the size, the default is 2 x 1 M reads at row_len 160).
per_read UMIs of 8 bases: both names of a pair take ":" R1's 8 bases "_" R2's 8 bases in front of their first space, the windows start behind the UMI.  Every row
is kept, so both calls read the same names.  Warmed up, alternating and repeated; the stage times are those of rfq_last_timings:
  plain     tag=None: select:names is what the names writer takes today
  tagged    the default formulation: select:tagplan + select:names
  general   RFQ_TAG=general: select:names (a thread per output name, byte by byte)
The yardstick is the BYTE ratio of the two blobs' traffic: the plain writer reads and writes the input name bytes N (2 N); the tagged one reads N, writes N + X
(X: the bytes inserted), and plan and records move - per output row - the name up to its place (read once more: at most N in all), a table entry, two offsets and
the unit's two windows (16 + 16 + 2 x 12 bytes), the parts (X at most), the record written (96 bytes) and what the writer reads of it (8 + |X|).
One JSON line: ms (median, min, all) per case and stage, the measured ratio (tagplan + names) / plain names and the byte ratio beside it.  Not gated: exit status 0.
    python tools/tag_bench.py [--pairs N] [--reps K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=160)
    ap.add_argument("--umi-len", type=int, default=8)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd import _capi as A
    from repaq_amd.tensors import fastq_to_tensors
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    L = args.row_len
    t = fastq_to_tensors(codec, t1, t2, paired=PE_TWO_FILES, row_len=L)
    del t1, t2
    n = t["lens"].numel()
    assert n == 2 * args.pairs
    ts = torch.zeros_like(t["lens"]); tl = torch.clamp(t["lens"], max=args.umi_len).contiguous(); start = tl.clone()
    rows = (n, L, t["bases"].data_ptr(), t["quals"].data_ptr(), t["lens"].data_ptr(), t["names"].data_ptr(), t["names"].numel(), t["name_off"].data_ptr())
    sel = dict(d_start=start.data_ptr(), pairs=True, min_len=0, codes=True)
    tag = dict(d_tag_start=ts.data_ptr(), d_tag_len=tl.data_ptr(), at=A.TAG_AT_SPACE)
    N = t["names"].numel()
    outs = {}
    for case, tg in (("plain", None), ("tagged", tag)):
        q = codec.select_rows(*rows, tag=tg, **sel)
        m, nl = int(q.n_rows), int(q.names_len)
        assert m == n
        o = dict(bases=torch.empty((m, L), dtype=torch.uint8, device=dev), quals=torch.empty((m, L), dtype=torch.uint8, device=dev), lens=torch.empty((m,), dtype=torch.int32, device=dev),
                 names=torch.empty((nl,), dtype=torch.uint8, device=dev), off=torch.empty((m + 1,), dtype=torch.int64, device=dev))
        outs[case] = (o, dict(row_len=L, out_bases=o["bases"].data_ptr(), bases_cap=m * L, out_quals=o["quals"].data_ptr(), quals_cap=m * L, out_lens=o["lens"].data_ptr(), lens_cap=m,
                              out_names=o["names"].data_ptr(), names_cap=nl, out_name_off=o["off"].data_ptr(), off_cap=m + 1), nl)
    X = outs["tagged"][2] - N

    def run(case, option):
        codec.set_option("RFQ_TAG", option)
        codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        try:
            codec.select_rows(*rows, tag=None if case == "plain" else tag, **sel, **outs[case][1])
            return codec.timings()
        finally:
            codec.set_stream(None); codec.set_option("RFQ_TAG", None)
    runs = {"plain": lambda: run("plain", None), "tagged": lambda: run("tagged", None), "general": lambda: run("tagged", "general")}
    for _ in range(args.warmup):
        runs["tagged"]()
        by_plan = outs["tagged"][0]["names"].clone()
        runs["general"]()
        assert torch.equal(by_plan, outs["tagged"][0]["names"]), "the formulations give different blobs"
        runs["plain"]()
    assert torch.equal(outs["plain"][0]["names"], t["names"])
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); st = f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            for name, v in st:
                stages[k].setdefault(name, []).append(v)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"tool": "tag_bench", "workload": "rows of synthetic NovaSeq PE150 (fqgen profile 1, %d pairs, seed %d) at row_len %d, names of %.1f bytes; per_read UMIs of %d, every row kept"
           % (args.pairs, args.seed, L, N / n, args.umi_len), "rows": n, "name_bytes_in": N, "name_bytes_out": outs["tagged"][2], "tag_bytes": X, "reps": args.reps}
    for k in runs:
        out[k] = {"ms_median": round(med(ms[k]), 3), "ms_min": round(min(ms[k]), 3), "stages_ms_median": {a: round(med(b), 4) for a, b in stages[k].items()},
                  "stages_ms_min": {a: round(min(b), 4) for a, b in stages[k].items()}, "names_ms_all": [round(x, 4) for x in stages[k]["select:names"]]}
    plain = out["plain"]["stages_ms_median"]["select:names"]
    tagged = out["tagged"]["stages_ms_median"]["select:tagplan"] + out["tagged"]["stages_ms_median"]["select:names"]
    moved = (N + N + X) + (N + n * (16 + 16 + 24) + X + n * 96 + n * 8 + X)
    out["measured_ratio"] = round(tagged / plain, 3)
    out["writer_alone_ratio"] = round(out["tagged"]["stages_ms_median"]["select:names"] / plain, 3)
    out["general_ratio"] = round(out["general"]["stages_ms_median"]["select:names"] / plain, 3)
    out["byte_ratio"] = round(moved / (2 * N), 3)
    out["plain_names_spread"] = round(max(stages["plain"]["select:names"]) / min(stages["plain"]["select:names"]), 3)
    print(json.dumps(out), flush=True)
    codec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
