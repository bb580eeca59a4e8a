"""List-major IVF at a general dimension against exact brute force on the same rows: device time per 1024 queries.

    python scripts/ivf_nd_bench.py [--dims 96,384,768] [--rows 1000000] [--nlist 1024] [--nprobe 8,32] [--groups 4] [--reps 5]

Data: synth_sift rows (integer valued) at every dimension, nlist sampled rows as centroids, every row assigned to its
nearest centroid through the library's own brute force (a timing index, not a trained one).  Queries: `groups` groups of
1024 distinct synth_sift rows of another seed (32 batches of 32), k = 10.  The yardstick is BruteForceIndex on the same rows
(vs_bf_create_nd, fp32 rows, search_dev_multi), alternated with the IVF calls in the same process; a timed window is all
groups of one path between two device events, reported per 1024 queries, every repeat listed.  recall@10 is IVF against
that exact result.  bytes_ratio is the expectation to compare against: brute force reads N rows per 32 queries, the list
scan group_q * nprobe / 16 blocks of N / nlist rows.  Each dimension runs in a process of its own; one JSON line per
measurement.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GROUP_Q, B, K = 1024, 32, 10


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    base = pkg.synth_sift(a.rows, seed=1, dim=dim)
    q = pkg.synth_sift(a.groups * GROUP_Q, seed=2, dim=dim)
    rng = np.random.default_rng(3)
    cents = np.ascontiguousarray(base[np.sort(rng.choice(a.rows, a.nlist, replace=False))])

    # assignment: the nearest centroid of every row, 1024 rows per call, through the library's brute force
    assign = np.empty(a.rows, dtype=np.int32)
    with pkg.BruteForceIndex(cents) as cidx:
        cidx.set_precision(1)
        step = GROUP_Q * 64
        oi = torch.empty((step, 2), dtype=torch.int32, device=dev)
        od = torch.empty((step, 2), dtype=torch.float32, device=dev)
        fl = torch.empty((step,), dtype=torch.int32, device=dev)
        for r0 in range(0, a.rows, step):
            chunk = torch.from_numpy(base[r0:r0 + step]).to(dev)
            n = chunk.shape[0]
            for c0 in range(0, n, GROUP_Q):
                full, rem = divmod(min(GROUP_Q, n - c0), B)
                if full:
                    cidx.search_dev_multi(chunk[c0].data_ptr(), full, B, 1, oi[c0].data_ptr(), od[c0].data_ptr(), fl[c0].data_ptr(), st)
                if rem:  # the ragged tail: one short batch
                    t0 = c0 + full * B
                    cidx.search_dev_multi(chunk[t0].data_ptr(), 1, rem, 1, oi[t0].data_ptr(), od[t0].data_ptr(), fl[t0].data_ptr(), st)
            torch.cuda.synchronize()
            assign[r0:r0 + n] = oi[:n, 0].cpu().numpy()
            del chunk
    vr, off, r2o = pkg.ivf_layout_from_assignment(base, assign, a.nlist)
    sizes = np.diff(off)
    print(json.dumps({"what": "index", "dim": dim, "rows": a.rows, "nlist": a.nlist, "list_min": int(sizes.min()),
                      "list_mean": float(sizes.mean()), "list_max": int(sizes.max())}), flush=True)

    qd = torch.from_numpy(q).to(dev)
    nbg = GROUP_Q // B
    nprobes = [int(x) for x in a.nprobe.split(",")]
    with pkg.BruteForceIndex(base) as bf, pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off,
                                                       reorder_to_original=r2o) as ivf:
        del vr
        bf.set_precision(1)
        bi = torch.empty((a.groups * GROUP_Q, K + 1), dtype=torch.int32, device=dev)
        bd = torch.empty((a.groups * GROUP_Q, K + 1), dtype=torch.float32, device=dev)
        bfl = torch.empty((a.groups * GROUP_Q,), dtype=torch.int32, device=dev)
        ii = torch.empty((a.groups * GROUP_Q, K), dtype=torch.int32, device=dev)
        idd = torch.empty((a.groups * GROUP_Q, K), dtype=torch.float32, device=dev)

        def run_bf():
            for g in range(a.groups):
                o = g * GROUP_Q
                bf.search_dev_multi(qd[o].data_ptr(), nbg, B, K, bi[o].data_ptr(), bd[o].data_ptr(), bfl[o].data_ptr(), st)

        def run_ivf(nprobe):
            for g in range(a.groups):
                o = g * GROUP_Q
                ivf.search_dev_multi(qd[o].data_ptr(), nbg, B, K, nprobe, ii[o].data_ptr(), idd[o].data_ptr(), st)

        def timed(f, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(*args)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.groups  # us per 1024 queries

        paths = [("bf", run_bf, ())] + [(f"ivf_nprobe{p}", run_ivf, (p,)) for p in nprobes]
        recall = {}
        for name, f, args in paths:  # warm-up of every path, and the recall of the IVF ones
            f(*args)
            f(*args)
            torch.cuda.synchronize()
            if name == "bf":
                exact = bi[:, :K].cpu().numpy()
            else:
                got = ii.cpu().numpy()
                recall[name] = float(np.mean([len(set(got[i]) & set(exact[i])) / K for i in range(len(exact))]))
        us = {name: [] for name, _, _ in paths}
        for _ in range(a.reps):
            for name, f, args in paths:
                us[name].append(timed(f, *args))
        med = {n: sorted(v)[len(v) // 2] for n, v in us.items()}
        for name, _, args in paths:
            rec = {"what": "us_per_1024_queries", "path": name, "dim": dim, "rows": a.rows, "nlist": a.nlist, "k": K,
                   "us": [round(u, 1) for u in us[name]], "median_us": round(med[name], 1)}
            if args:
                rec["recall_at_10"] = round(recall[name], 4)
                rec["speedup_vs_bf"] = round(med["bf"] / med[name], 2)
                rec["bytes_ratio"] = round((GROUP_Q / B) / (GROUP_Q * args[0] / 16.0 / a.nlist), 2)
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,384,768")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="8,32")
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a, a.one)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--nlist", str(a.nlist), "--nprobe", a.nprobe,
           "--groups", str(a.groups), "--reps", str(a.reps)]
    for dim in [int(x) for x in a.dims.split(",")]:
        r = subprocess.run(cmd + ["--one", str(dim)], timeout=900)
        if r.returncode != 0:  # a failed or faulted step ends the run: nothing more is started on the GPU
            sys.exit(r.returncode if r.returncode > 0 else 1)


if __name__ == "__main__":
    main()
