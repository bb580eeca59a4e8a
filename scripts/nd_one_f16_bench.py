"""The single-call scan on float16 rows (scan_one_nd_f16_kernel) at N = 1 M gaussian rows rounded to float16,
k = 5, one batch of B = 1 and of B = 16 queries per call, per dimension, in one process and one session:

    one     a from_f16 index, default route (one scan_one_nd_f16_kernel launch per call)
    off     a from_f16 index created under VSEARCH_ND_ONE_F16=0 (per-batch route: nd_prep_kernel, slot reset,
            scan_nd_f16_kernel, merge) -- the behaviour before the route existed
    off2    the same index measured a second time in every repeat: the spread of the yardstick
    f32     the rows widened to float in a BruteForceIndex (scan_one_nd_kernel; at dim 128 the specialised index and its
            scan_one_kernel), for scale

Per leg and repeat: microseconds per call by HIP events over back-to-back calls (a window of about 0.1 s after warm-up
calls), and the delivered row bytes (2 N dim_h; 4 N dim_p for f32) per second as a fraction of the 8 TB/s HBM peak from
the best repeat.  The legs alternate inside every repeat.  Before anything is timed, the outputs (ids, distance bits,
flags) of four calls are compared across all legs: a leg that answers differently ends the run.

    python scripts/nd_one_f16_bench.py [--dims 96,128,384,768,1024,2048] [--rows 1000000] [--reps 3] > profiles/nd_one_f16_bench.txt

One JSON line per (dimension, B, leg) with every repeat and min / max, then one summary line per (dimension, B)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # as bench.py
K = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128,384,768,1024,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,16")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for dim in [int(x) for x in a.dims.split(",")]:
        gen = torch.Generator(device=dev).manual_seed(dim)
        half = torch.randn((a.rows, dim), generator=gen, device=dev).half()
        base = half.cpu().numpy()
        wide = half.float().cpu().numpy()
        qd = torch.randn((64 * 16, dim), generator=gen, device=dev)
        del half
        idx = {"one": pkg.BruteForceIndex.from_f16(base)}
        os.environ["VSEARCH_ND_ONE_F16"] = "0"
        try:
            idx["off"] = pkg.BruteForceIndex.from_f16(base)
        finally:
            del os.environ["VSEARCH_ND_ONE_F16"]
        idx["off2"] = idx["off"]
        idx["f32"] = pkg.BruteForceIndex(wide)
        del base, wide
        oi = torch.zeros((16, K + 1), dtype=torch.int32, device=dev)
        od = torch.zeros((16, K + 1), dtype=torch.float32, device=dev)
        fl = torch.zeros((16,), dtype=torch.int32, device=dev)

        def call(ix, B, i):
            ix.search_dev(qd.data_ptr() + (i % 64) * B * dim * 4, B, K, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)

        def measure(ix, B):
            for i in range(8):
                call(ix, B, i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(16):
                call(ix, B, i)
            torch.cuda.synchronize()
            n = int(min(2000, max(64, 0.1 / max((time.perf_counter() - t0) / 16, 1e-6))))  # a window of about 0.1 s
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                call(ix, B, i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n

        dim_h, dim_p = (dim + 31) // 32 * 32, (dim + 15) // 16 * 16
        for B in [int(x) for x in a.batches.split(",")]:
            outs = {}
            idx["one"].one_f16_stats(True)
            for name in ("one", "off", "f32"):
                got = []
                for i in range(4):  # (forwards and backwards walks)
                    call(idx[name], B, i)
                    torch.cuda.synchronize()
                    got += [t[:B].cpu().numpy().tobytes() for t in (oi, od, fl)]
                outs[name] = b"".join(got)
            if not (outs["one"] == outs["off"] == outs["f32"]):
                raise SystemExit(f"dim {dim} B {B}: the legs answer differently")
            assert idx["one"].one_f16_stats(True) == 4 and idx["off"].one_f16_stats() == 0
            res = {name: [] for name in idx}
            for _ in range(a.reps):
                for name in idx:
                    res[name].append(measure(idx[name], B))
            for name, us in res.items():
                row_bytes = 4 * dim_p if name == "f32" else 2 * dim_h
                print(json.dumps({"dim": dim, "rows": a.rows, "B": B, "k": K, "leg": name, "us_per_call": [round(x, 2) for x in us],
                                  "us_min": round(min(us), 2), "us_max": round(max(us), 2), "row_bytes": row_bytes,
                                  "hbm_frac_best": round(a.rows * row_bytes / (min(us) * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                  "same_outputs": True}), flush=True)
            off = res["off"] + res["off2"]
            print(json.dumps({"dim": dim, "B": B, "summary": "one against off",
                              "speedup_worst": round(min(off) / max(res["one"]), 3), "speedup_best_of_each": round(min(off) / min(res["one"]), 3),
                              "spread_one": round(max(res["one"]) / min(res["one"]) - 1, 3), "spread_off": round(max(off) / min(off) - 1, 3),
                              "faster_beyond_spread": max(res["one"]) < min(off),
                              "f32_over_one": round(min(res["f32"]) / min(res["one"]), 3)}), flush=True)
        for name in ("one", "off", "f32"):
            idx[name].close()
        del qd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
