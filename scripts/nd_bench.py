"""General-dimension brute force at N = 1 M rows: device time per batch of the per-batch scan (64 batches of 32 queries per
call, k = 5, fp32 rows) and the delivered row bytes 4 N dim_p per second as a fraction of the HBM peak, per dimension; and
(--host) host-to-host QPS of search / search_topk with tie replay at one dimension.  One JSON line per measurement; every
repeat is listed, not only the best.

    python scripts/nd_bench.py [--dims 96,128,256,384,768,960,1024,2048] [--rows 1000000] [--reps 5]
    python scripts/nd_bench.py --host --dims 960 --k 5,100 --nq 1000
    python scripts/nd_bench.py --u8 [--dims 96,256,960,2048]

--u8 is the byte leg: the same shapes on an index made from uint8 rows (BruteForceIndex.from_u8), precision 1 (fp32 rows,
scan_nd_kernel) and precision 2 (byte rows, scan_nd_i8_kernel) alternating on the same index in the same process; the byte
scan's delivered bytes are N dim_b, dim_b = dim rounded up to 64.  --u8 --metric ip measures the inner-product byte index
(from_u8(metric=METRIC_IP)): its byte scan and its fp32 rows alternating, between two legs of the L2 byte scan of a from_u8
index on the same rows (profiles/nd_u8_ip_bench.txt: --u8 --metric ip --dims 96,128,256,960,2048).

Each dimension runs in a process of its own.  128 is measured twice, alternating: the specialised per-batch scan_kernel
(VSEARCH_STREAM=0: streaming scans off) and the general kernel on the same data (VSEARCH_ND_FORCE=1).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0  # as bench.py


def _data(rows, dim, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=dtype)
    step = max(1, (1 << 26) // dim)
    for r0 in range(0, rows, step):
        out[r0:r0 + step] = rng.integers(0, 64, size=(min(step, rows - r0), dim), dtype=np.uint8)
    return out


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    tag = os.environ.get("ND_BENCH_TAG", "general")
    if a.u8:
        return one_u8(a, dim, pkg, torch)
    base = _data(a.rows, dim, 1)
    with pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        if a.host:
            q = _data(a.nq, dim, 2)
            for k in [int(x) for x in a.k.split(",")]:
                idx.search_topk(q[:64], k)
                qps = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    idx.search_topk(q, k)
                    qps.append(a.nq / (time.perf_counter() - t0))
                print(json.dumps({"what": "host_qps", "dim": dim, "rows": a.rows, "nq": a.nq, "k": k, "qps": [round(x, 1) for x in qps]}), flush=True)
            return
        dev = torch.device("cuda:0")
        nb, B, k = 64, 32, 5
        qd = torch.from_numpy(_data(nb * B, dim, 2)).to(dev)
        oi = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
        od = torch.empty((nb * B, k + 1), dtype=torch.float32, device=dev)
        fl = torch.empty((nb * B,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda: idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.reps):
            idx.prof_enable(True)
            call()
            torch.cuda.synchronize()
            ms, _n = idx.prof_read(0)
            idx.prof_enable(False)
            us.append(ms * 1e3 / nb)
        dim_p = dim if tag == "scan_kernel" else (dim + 15) // 16 * 16
        frac = [4.0 * a.rows * dim_p / (u * 1e-6) / 1e9 / HBM_PEAK_GBS for u in us]
        print(json.dumps({"what": "scan_us_per_batch", "kernel": tag, "dim": dim, "dim_p": dim_p, "rows": a.rows,
                          "us_per_batch": [round(u, 2) for u in us], "hbm_frac": [round(f, 4) for f in frac],
                          "tflops": round(2.0 * B * a.rows * dim / (min(us) * 1e-6) / 1e12, 2)}), flush=True)


def one_u8_ip(a, dim, pkg, torch):
    """--u8 --metric ip: the inner-product byte index (from_u8(metric=METRIC_IP)) -- its byte scan (precision 2) and its fp32
    rows (precision 1), alternating -- between two legs of the L2 byte scan of a from_u8 index on the same rows."""
    base = _data(a.rows, dim, 1, np.uint8)
    with pkg.BruteForceIndex.from_u8(base) as l2, pkg.BruteForceIndex.from_u8(base, metric=pkg.METRIC_IP) as ip:
        del base
        dev = torch.device("cuda:0")
        nb, B, k = 64, 32, 5
        qd = torch.from_numpy(_data(nb * B, dim, 2)).to(dev)
        oi = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
        od = torch.empty((nb * B, k + 1), dtype=torch.float32, device=dev)
        fl = torch.empty((nb * B,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def timed(idx, prec, warm=0):
            idx.set_precision(prec)
            for _ in range(warm):
                idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
            idx.prof_enable(True)
            idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
            torch.cuda.synchronize()
            ms, _n = idx.prof_read(0)
            idx.prof_enable(False)
            assert not bool((fl == 2).any()), "a batch was refused by the byte scan"
            return ms * 1e3 / nb

        # warm-up of the three kernels; the inner-product byte scan must agree with the fp32 rows to the bit
        timed(l2, 2, warm=2)
        got = {}
        for prec in (1, 2):
            timed(ip, prec, warm=2)
            got[prec] = (od.clone(), oi.clone())
        assert torch.equal(got[1][0], got[2][0]) and torch.equal(got[1][1], got[2][1]), "byte and fp32 scores differ"
        us = {"l2_i8_before": [timed(l2, 2) for _ in range(a.reps)], "ip_fp32": [], "ip_i8": []}
        for _ in range(a.reps):
            us["ip_fp32"].append(timed(ip, 1))
            us["ip_i8"].append(timed(ip, 2))
        us["l2_i8_after"] = [timed(l2, 2) for _ in range(a.reps)]
        dim_p, dim_b = (dim + 15) // 16 * 16, (dim + 63) // 64 * 64
        for leg, row_bytes in (("l2_i8_before", dim_b), ("ip_fp32", 4 * dim_p), ("ip_i8", dim_b), ("l2_i8_after", dim_b)):
            frac = [a.rows * float(row_bytes) / (u * 1e-6) / 1e9 / HBM_PEAK_GBS for u in us[leg]]
            print(json.dumps({"what": "scan_us_per_batch", "leg": leg, "dim": dim, "row_bytes": row_bytes, "rows": a.rows,
                              "us_per_batch": [round(u, 2) for u in us[leg]], "hbm_frac": [round(f, 4) for f in frac]}), flush=True)
        med = {leg: sorted(v)[len(v) // 2] for leg, v in us.items()}
        print(json.dumps({"what": "ip_i8_vs_fp32", "dim": dim, "rows": a.rows, "median_us_ip_fp32": round(med["ip_fp32"], 2),
                          "median_us_ip_i8": round(med["ip_i8"], 2), "speedup": round(med["ip_fp32"] / med["ip_i8"], 3),
                          "median_us_l2_i8_before": round(med["l2_i8_before"], 2), "median_us_l2_i8_after": round(med["l2_i8_after"], 2)}),
              flush=True)


def one_u8(a, dim, pkg, torch):
    if a.metric == "ip":
        return one_u8_ip(a, dim, pkg, torch)
    base = _data(a.rows, dim, 1, np.uint8)
    with pkg.BruteForceIndex.from_u8(base) as idx:
        del base
        dev = torch.device("cuda:0")
        nb, B, k = 64, 32, 5
        qd = torch.from_numpy(_data(nb * B, dim, 2)).to(dev)
        oi = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
        od = torch.empty((nb * B, k + 1), dtype=torch.float32, device=dev)
        fl = torch.empty((nb * B,), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda: idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
        us = {1: [], 2: []}
        dists = {}
        for prec in (1, 2):  # warm-up of both kernels; the byte scan must have run every batch and agree with fp32
            idx.set_precision(prec)
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            assert not bool((fl == 2).any()), "a batch was refused by the byte scan"
            dists[prec] = od.clone()
        assert torch.equal(dists[1], dists[2]), "byte and fp32 distances differ"
        for _ in range(a.reps):
            for prec in (1, 2):
                idx.set_precision(prec)
                idx.prof_enable(True)
                call()
                torch.cuda.synchronize()
                ms, _n = idx.prof_read(0)
                idx.prof_enable(False)
                us[prec].append(ms * 1e3 / nb)
        dim_p, dim_b = (dim + 15) // 16 * 16, (dim + 63) // 64 * 64
        for prec, kernel, row_bytes in ((1, "fp32", 4.0 * dim_p), (2, "i8", 1.0 * dim_b)):
            frac = [a.rows * row_bytes / (u * 1e-6) / 1e9 / HBM_PEAK_GBS for u in us[prec]]
            print(json.dumps({"what": "scan_us_per_batch", "index": "from_u8", "kernel": kernel, "precision": prec, "dim": dim,
                              "row_bytes": int(row_bytes), "rows": a.rows, "us_per_batch": [round(u, 2) for u in us[prec]],
                              "hbm_frac": [round(f, 4) for f in frac]}), flush=True)
        med = {p: sorted(us[p])[len(us[p]) // 2] for p in us}
        print(json.dumps({"what": "i8_vs_fp32", "dim": dim, "rows": a.rows, "median_us_fp32": round(med[1], 2),
                          "median_us_i8": round(med[2], 2), "speedup": round(med[1] / med[2], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128,256,384,768,960,1024,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--u8", action="store_true", help="byte leg: from_u8 index, precision 2 against 1")
    ap.add_argument("--metric", choices=("l2", "ip"), default="l2", help="with --u8: ip = the inner-product byte index between two L2 legs")
    ap.add_argument("--k", default="5,100")
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a, a.one)
        return
    base_cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--reps", str(a.reps), "--k", a.k, "--nq", str(a.nq)]
    if a.host:
        base_cmd.append("--host")
    if a.u8:
        base_cmd += ["--u8", "--metric", a.metric]
    for dim in [int(x) for x in a.dims.split(",")]:
        runs = [({}, "general")]
        if dim == 128 and not a.host and not a.u8:  # alternate the yardstick and the forced general kernel
            y, g = ({"VSEARCH_STREAM": "0"}, "scan_kernel"), ({"VSEARCH_ND_FORCE": "1"}, "general")
            runs = [y, g, y, g]
        for env, tag in runs:
            e = dict(os.environ)
            e.update(env)
            e["ND_BENCH_TAG"] = tag
            r = subprocess.run(base_cmd + ["--one", str(dim)], env=e, timeout=900)
            if r.returncode != 0:  # a failed or faulted step ends the run: nothing more is started on the GPU
                sys.exit(r.returncode if r.returncode > 0 else 1)


if __name__ == "__main__":
    main()
