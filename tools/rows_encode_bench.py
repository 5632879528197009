"""rfq_rows_to_text / rfq_encode_rows against their yardsticks on one context (configs[2]-shaped input: synthetic NovaSeq PE150, -k 1000, fqgen
profile 1, seed 3 - bench.py's generator path).  The rows are decode_tensors' of the encoded image (row_len 150 or --row-len, codes), the names are
packed on the device from the text.  Warmed up, alternating and repeated, timed with device events:
  (a) rfq_encode_batch on the text itself (RFQ_PE_TWO_FILES)
  (b) rfq_encode_rows on the rows of the same reads - (b) - (a) is what the text in between costs
  (c) rfq_rows_to_text into preallocated caller buffers; its stages rows_sizes and rows_text from rfq_last_timings
  (d) one hipMemcpy device-to-device of as many bytes as the two texts hold - the yardstick of k_rows_text
One JSON line: ms (median, min) of each, the stage medians, bytes of text per second of k_rows_text and of the copy, and their ratio.
    python tools/rows_encode_bench.py [--pairs N] [--reps K] [--row-len L]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def names_on_device(torch, t1, t2):
    """the name lines of two texts in HBM, interleaved (R1 of pair k, then its R2), as (blob, offsets)"""
    dev = t1.device

    def name_lines(t, base):
        nl = torch.nonzero(t == 10).flatten()
        starts = torch.cat([torch.zeros(1, dtype=nl.dtype, device=dev), nl + 1])
        n = nl.numel() // 4
        return starts[0:4 * n:4] + base, nl[0:4 * n:4] - starts[0:4 * n:4]
    s1, l1 = name_lines(t1, 0); s2, l2 = name_lines(t2, t1.numel())
    start = torch.stack([s1, s2], 1).flatten(); ln = torch.stack([l1, l2], 1).flatten()
    off = torch.zeros(ln.numel() + 1, dtype=torch.int64, device=dev); off[1:] = torch.cumsum(ln, 0)
    row = torch.repeat_interleave(torch.arange(ln.numel(), device=dev), ln)
    src = start[row] + (torch.arange(int(off[-1]), device=dev) - off[row])
    return torch.cat([t1, t2])[src].contiguous(), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=11_200_000)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--row-len", type=int, default=150)
    args = ap.parse_args()
    import torch
    import _oracle as O
    from repaq_amd import RfqCodec, PE_TWO_FILES
    from repaq_amd.tensors import decode_tensors
    dev = torch.device("cuda:0")
    codec = RfqCodec(device=0)
    a1, a2 = O.gen_np(O.NOVA_PE150, args.pairs, seed=args.seed)
    n1, n2 = int(a1.size), int(a2.size)
    t1 = torch.from_numpy(a1).to(dev); t2 = torch.from_numpy(a2).to(dev)
    del a1, a2
    r = codec.encode(t1.data_ptr(), n1, t2.data_ptr(), n2, PE_TWO_FILES, 1_000_000)
    rfq_len = int(r.rfq_len)
    rfq = torch.empty(rfq_len, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(rfq.data_ptr()), C.c_void_p(r.d_rfq), rfq_len))
    rows = decode_tensors(codec, rfq, row_len=args.row_len)
    blob, off = names_on_device(torch, t1, t2)
    torch.cuda.synchronize()
    n, L = int(rows["lens"].numel()), int(rows["bases"].shape[1])
    ra = (n, L, rows["bases"].data_ptr(), rows["quals"].data_ptr(), rows["lens"].data_ptr(), blob.data_ptr(), blob.numel(), off.data_ptr())
    o1 = torch.empty(n1 + 64, dtype=torch.uint8, device=dev); o2 = torch.empty(n2 + 64, dtype=torch.uint8, device=dev)
    cp = torch.empty(n1 + n2, dtype=torch.uint8, device=dev)
    codec.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ok = {}

    def run_a():
        codec.clearHeader()
        x = codec.encode(t1.data_ptr(), n1, t2.data_ptr(), n2, PE_TWO_FILES, 1_000_000)
        ok["a"] = int(x.rfq_len)

    def run_b():
        codec.clearHeader()
        x = codec.encode_rows(*ra, paired=PE_TWO_FILES, codes=True, chunk_bases=1_000_000)
        ok["b"] = int(x.rfq_len)

    def run_c():
        codec.rows_to_text(*ra, paired=PE_TWO_FILES, codes=True, d_out1=o1.data_ptr(), cap1=n1 + 64, d_out2=o2.data_ptr(), cap2=n2 + 64)

    def run_d():
        codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(cp.data_ptr()), C.c_void_p(o1.data_ptr()), n1))
        codec._check(codec._L.rfq_copy_d2d(codec._h, C.c_void_p(cp.data_ptr() + n1), C.c_void_p(o2.data_ptr()), n2))
    runs = {"a_encode_text": run_a, "b_encode_rows": run_b, "c_rows_to_text": run_c, "d_copy_d2d": run_d}
    for _ in range(args.warmup):
        for f in runs.values():
            f()
    assert ok["a"] == ok["b"] == rfq_len and torch.equal(o1[:n1], t1) and torch.equal(o2[:n2], t2)
    ms = {k: [] for k in runs}; stages = {k: {} for k in runs}
    for _ in range(args.reps):
        for k, f in runs.items():
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record(); f(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            if k in ("b_encode_rows", "c_rows_to_text"):
                for name, t in codec.timings():
                    stages[k].setdefault(name, []).append(t)

    def med(v):
        s = sorted(v); return s[len(s) // 2]
    text_bytes = n1 + n2
    out = {"tool": "rows_encode_bench", "workload": "configs[2]-shaped: synthetic NovaSeq PE150 2 x %.2f GB (fqgen profile 1, %d pairs, seed %d), -k 1000" % (n1 / 1e9, args.pairs, args.seed),
           "rows": n, "row_len": L, "text_bytes": text_bytes, "rfq_bytes": rfq_len, "reps": args.reps}
    for k, v in ms.items():
        out[k] = {"ms_median": round(med(v), 3), "ms_min": round(min(v), 3), "ms_all": [round(x, 3) for x in v],
                  "stages_ms_median": {a: round(med(b), 3) for a, b in stages[k].items()}}
    wt = out["c_rows_to_text"]["stages_ms_median"].get("rows_text", 0.0)
    out["rows_text_GBps"] = round(text_bytes / (wt * 1e6), 1) if wt else None
    out["copy_d2d_GBps"] = round(text_bytes / (out["d_copy_d2d"]["ms_median"] * 1e6), 1)
    out["rows_text_over_copy"] = round(out["rows_text_GBps"] / out["copy_d2d_GBps"], 3) if wt else None
    out["encode_rows_over_encode_text"] = round(out["b_encode_rows"]["ms_median"] / out["a_encode_text"]["ms_median"], 3)
    print(json.dumps(out), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
