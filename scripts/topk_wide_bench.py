"""Wide-k brute force on the SIFT-1M shape (synth_sift, 1 M rows, 10 000 queries): device QPS of
vs_bf_search_topk_dev_multi (batches of 32, 32 batches per launch), host-to-host QPS of vs_bf_search_topk with its tie
replay, and (--stats: a second process with VSEARCH_TOPW_STATS=1) the flagged fraction, candidates per query and how many
batches overflowed into the dense path.  One JSON line per k.

    python scripts/topk_wide_bench.py [--k 10,50,100,128] [--nq 10000] [--rows 1000000] [--stats]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="10,50,100,128")
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats", action="store_true", help="also run each k once more with VSEARCH_TOPW_STATS=1")
    ap.add_argument("--host-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    base = pkg.synth_sift(a.rows, seed=1)
    q = pkg.synth_sift(a.nq, seed=2)
    ks = [int(x) for x in a.k.split(",")]
    with pkg.BruteForceIndex(base) as idx:
        for k in ks:
            rec = {"k": k, "rows": a.rows, "nq": a.nq}
            if not a.host_only:
                dev = torch.device("cuda:0")
                nb = a.nq // 32
                qd = torch.from_numpy(q[:nb * 32]).to(dev)
                oi = torch.empty((nb * 32, k + 1), dtype=torch.int32, device=dev)
                od = torch.empty((nb * 32, k + 1), dtype=torch.float32, device=dev)
                fl = torch.empty((nb * 32,), dtype=torch.int32, device=dev)
                st = torch.cuda.current_stream().cuda_stream
                call = lambda: idx.search_topk_dev_multi(qd.data_ptr(), nb, 32, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
                call()
                torch.cuda.synchronize()
                best = 1e30
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    torch.cuda.synchronize()
                    best = min(best, time.perf_counter() - t0)
                rec["device_qps"] = nb * 32 / best
                rec["device_flagged_frac"] = float((fl.cpu().numpy() != 0).mean())
            idx.search_topk(q[:64], k)  # warm-up: lazy buffers, kernel code
            best_tm = None
            for _ in range(a.reps):
                tm = pkg.Timing()
                t0 = time.perf_counter()
                idx.search_topk(q, k, tm)
                wall = time.perf_counter() - t0
                if best_tm is None or wall < best_tm[0]:
                    best_tm = (wall, tm.total_ms, tm.fine_search_ms, tm.tie_resolve_ms, tm.tie_queries)
            wall, total_ms, fine_ms, tie_ms, tie_q = best_tm
            rec.update(host_qps=a.nq / wall, total_ms=total_ms, search_ms=fine_ms, tie_resolve_ms=tie_ms,
                       flagged_frac=tie_q / a.nq)
            print(json.dumps(rec), flush=True)
    if a.stats:
        env = dict(os.environ, VSEARCH_TOPW_STATS="1")
        for k in ks:
            if k <= 15:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--k", str(k), "--nq", str(a.nq), "--rows", str(a.rows),
                                "--reps", "1", "--host-only"], env=env, capture_output=True, text=True)
            lines = [ln for ln in r.stderr.splitlines() if ln.startswith("topw_stats")]
            print(json.dumps({"k": k, "stats": lines[-1] if lines else r.stderr[-500:]}), flush=True)


if __name__ == "__main__":
    main()
