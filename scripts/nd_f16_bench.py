"""The float16 brute-force index against the fp32 general index on the same rows widened, N = 1 M gaussian rows rounded to
float16, 64 batches of B = 32 queries per call, k = 5 (search_dev_multi) and k = 100 (search_topk_dev_multi): device time
per batch by HIP events, per dimension.  One JSON line per dimension and k; every repeat is listed.

    python scripts/nd_f16_bench.py [--dims 96,128,384,768,1024,2048] [--rows 1000000] [--reps 5] [--default-routes]

Each dimension runs in a process of its own, under VSEARCH_ND_FILTER=0 and VSEARCH_ND_ONE=0, so that both indexes run
their per-batch kernels (scan_nd_f16_kernel against scan_nd_kernel); --default-routes leaves the fp32 index its prefilter
and single-call routes instead (reported, nothing is claimed about them).  The two indexes live in the same process and
alternate repeat by repeat: f16, f32, f16, f32, ...  Row bytes delivered: 2 N dim_h against 4 N dim_p.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0  # as bench.py


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    rng = np.random.default_rng(dim)
    base = np.empty((a.rows, dim), dtype=np.float16)
    step = max(1, (1 << 25) // dim)
    for r0 in range(0, a.rows, step):
        base[r0:r0 + step] = rng.normal(0, 1, size=(min(step, a.rows - r0), dim))
    nb, B = 64, 32
    q = torch.from_numpy(rng.normal(0, 1, size=(nb * B, dim)).astype(np.float32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    with pkg.BruteForceIndex.from_f16(base) as h16, pkg.BruteForceIndex(base.astype(np.float32)) as f32:
        for k in (5, 100):
            ids = torch.empty((nb * B, k + 1), dtype=torch.int32, device="cuda")
            d = torch.empty((nb * B, k + 1), dtype=torch.float32, device="cuda")
            fl = torch.empty((nb * B,), dtype=torch.int32, device="cuda")

            def call(idx):
                f = idx.search_dev_multi if k <= 15 else idx.search_topk_dev_multi
                f(q.data_ptr(), nb, B, k, ids.data_ptr(), d.data_ptr(), fl.data_ptr(), s)

            us = {"f16": [], "f32": []}
            for name, idx in (("f16", h16), ("f32", f32)):  # warm-up: scratch allocation, code upload
                call(idx)
            torch.cuda.synchronize()
            for _ in range(a.reps):
                for name, idx in (("f16", h16), ("f32", f32)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(idx)
                    e1.record()
                    e1.synchronize()
                    us[name].append(round(e0.elapsed_time(e1) * 1000.0 / nb, 2))
            m16, m32 = float(np.median(us["f16"])), float(np.median(us["f32"]))
            dim_h, dim_p = (dim + 31) // 32 * 32, (dim + 15) // 16 * 16
            print(json.dumps({
                "dim": dim, "rows": a.rows, "k": k, "B": B, "batches": nb, "default_routes": bool(a.default_routes),
                "f16_us_per_batch": us["f16"], "f32_us_per_batch": us["f32"], "f16_median": m16, "f32_median": m32,
                "f32_over_f16": round(m32 / m16, 3),
                "f16_hbm_frac": round(2.0 * a.rows * dim_h / (m16 * 1e-6) / 1e9 / HBM_PEAK_GBS, 3) if k <= 15 else None,
                "f32_hbm_frac": round(4.0 * a.rows * dim_p / (m32 * 1e-6) / 1e9 / HBM_PEAK_GBS, 3) if k <= 15 else None,
            }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128,384,768,1024,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--default-routes", action="store_true")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a, a.one)
    for dim in [int(x) for x in a.dims.split(",")]:
        env = dict(os.environ)
        if not a.default_routes:
            env.update(VSEARCH_ND_FILTER="0", VSEARCH_ND_ONE="0")
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(dim), "--rows", str(a.rows), "--reps", str(a.reps)]
        if a.default_routes:
            cmd.append("--default-routes")
        subprocess.run(cmd, env=env, check=True, timeout=600)


if __name__ == "__main__":
    main()
