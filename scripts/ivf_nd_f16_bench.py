"""The float16 IVF index (IVFIndex.from_f16: vs_ivf_create_nd_f16, ivf_scan_nd_f16_kernel) against vs_ivf_create on the same
rows widened to float: N = 1 M gaussian rows rounded to float16, nlist 1024 from the library's builder, launch groups of 1024
queries (32 batches of 32, search_dev_multi), k = 10, nprobe 8 and 32, per dimension.

    python scripts/ivf_nd_f16_bench.py [--dims 96,384,768,2048] [--rows 1000000] [--nlist 1024] [--nprobe 8,32] [--reps 5]
                                       [--groups 4] [--build-iters 3] [--tag TEXT]

Each dimension runs in a process of its own.  The two indexes live in that process and alternate repeat by repeat (f16, f32,
f16, f32, ...); every repeat is listed, so each leg's spread can be read beside the ratio.  Per index and nprobe:
  us_per_group   : device time between two HIP events around --groups calls back to back, per 1024 queries;
  scan_us        : the list-scan launch alone (vs_prof_read window 1), per group, in passes of their own;
and once per dimension the device memory each index took (free memory before and after its creation) beside the row bytes
it should hold, N (2 dim_h + 4) against N (4 dim_p + 4), and whether the two indexes returned the same bits.
--tag is copied into every line (which build of the library ran).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    rng = np.random.default_rng(dim)
    base = np.empty((a.rows, dim), dtype=np.float16)
    step = max(1, (1 << 25) // dim)
    for r0 in range(0, a.rows, step):
        base[r0:r0 + step] = rng.normal(0, 1, size=(min(step, a.rows - r0), dim))
    vr, off, r2o, cents, iters = pkg.ivf_build(base.astype(np.float32), a.nlist, a.build_iters, 0.0, 42)
    del base
    rows_h = vr.astype(np.float16)
    assert np.array_equal(rows_h.astype(np.float32), vr)  # (the reordered rows are the input's rows)
    nb, B, k = 32, 32, 10
    q = torch.from_numpy(rng.normal(0, 1, size=(nb * B, dim)).astype(np.float32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    h16 = pkg.IVFIndex.from_f16(rows_h, cents, off, r2o)
    free1 = torch.cuda.mem_get_info()[0]
    f32 = pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o)
    free2 = torch.cuda.mem_get_info()[0]
    del vr, rows_h
    legs = (("f16", h16), ("f32", f32))
    out = {name: (torch.empty((nb * B, k), dtype=torch.int32, device="cuda"), torch.empty((nb * B, k), dtype=torch.float32, device="cuda"))
           for name, _ in legs}
    sizes = np.diff(off)
    dim_h, dim_p = (dim + 31) // 32 * 32, (dim + 15) // 16 * 16
    same = True
    with h16, f32:
        for nprobe in a.nprobe:
            def call(name, idx):
                idx.search_dev_multi(q.data_ptr(), nb, B, k, nprobe, out[name][0].data_ptr(), out[name][1].data_ptr(), s)

            for name, idx in legs:  # warm-up: code upload, clocks
                call(name, idx)
            torch.cuda.synchronize()
            same = same and torch.equal(out["f16"][0], out["f32"][0]) and torch.equal(out["f16"][1].view(torch.int32), out["f32"][1].view(torch.int32))
            us = {"f16": [], "f32": []}
            scan = {"f16": [], "f32": []}
            for _ in range(a.reps):
                for name, idx in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _g in range(a.groups):
                        call(name, idx)
                    e1.record()
                    e1.synchronize()
                    us[name].append(round(e0.elapsed_time(e1) * 1000.0 / a.groups, 1))
            for _ in range(a.reps):  # the list-scan launches alone, in passes of their own (the profiling events cost time)
                for name, idx in legs:
                    idx.prof_enable(True)
                    for _g in range(a.groups):
                        call(name, idx)
                    torch.cuda.synchronize()
                    ms, n = idx.prof_read(1)
                    idx.prof_enable(False)
                    scan[name].append(round(ms * 1000.0 / max(n, 1), 1))
            med = lambda v: float(np.median(v))
            print(json.dumps({
                "tag": a.tag, "dim": dim, "rows": a.rows, "nlist": int(len(sizes)), "build_iters": iters, "list_min": int(sizes.min()),
                "list_max": int(sizes.max()), "nprobe": nprobe, "k": k, "group_q": nb * B,
                "f16_us_per_group": us["f16"], "f32_us_per_group": us["f32"], "f16_scan_us": scan["f16"], "f32_scan_us": scan["f32"],
                "group_f32_over_f16": round(med(us["f32"]) / med(us["f16"]), 3), "scan_f32_over_f16": round(med(scan["f32"]) / med(scan["f16"]), 3),
            }), flush=True)
    print(json.dumps({
        "tag": a.tag, "what": "memory", "dim": dim, "rows": a.rows, "same_bits": bool(same),
        "f16_index_MiB": round((free0 - free1) / 2 ** 20, 1), "f32_index_MiB": round((free1 - free2) / 2 ** 20, 1),
        "f16_row_MiB_expected": round(a.rows * (2 * dim_h + 4) / 2 ** 20, 1), "f32_row_MiB_expected": round(a.rows * (4 * dim_p + 4) / 2 ** 20, 1),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,384,768,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--build-iters", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        a.nprobe = [int(x) for x in a.nprobe.split(",")]
        return one(a, a.one)
    for dim in [int(x) for x in a.dims.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(dim), "--rows", str(a.rows), "--nlist", str(a.nlist), "--nprobe", a.nprobe,
               "--reps", str(a.reps), "--groups", str(a.groups), "--build-iters", str(a.build_iters), "--tag", a.tag]
        subprocess.run(cmd, check=True, timeout=900)


if __name__ == "__main__":
    main()
