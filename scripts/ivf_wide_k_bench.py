"""Micro-benchmark of IVF search at wide k (17 <= k <= 128) on SIFT-1M-shaped data (nlist 1024, nprobe 32, 8 192 distinct
queries per call = one launch group of 256 batches of 32), beside k = 10 (the k <= 16 pipeline) for reference: device time
per call and QPS for both precisions.  Run it under rocprofv3 --kernel-trace --stats for the per-kernel times.
    python scripts/ivf_wide_k_bench.py [--nprobe 32] [--ks 10,100,128] [--precisions 0,1]
--stats: instead of timing, the wide-k pipeline's fill (VSEARCH_IVF_WIDEK_STATS: candidates per query, exactly ranked
queries, overflowed groups) per k and precision, and recall@100 over --recall-queries queries of the host call against
the ground truth that vsearch_bf --groundtruth writes."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--ks", default="10,100,128")
ap.add_argument("--precisions", default="0,1")
ap.add_argument("--stats", action="store_true")
ap.add_argument("--recall-queries", type=int, default=10000)
a = ap.parse_args()
if a.stats:
    os.environ["VSEARCH_IVF_WIDEK_STATS"] = "1"  # (read at the first wide-k call)
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge

pkg = ge.load_package()
B, NB = 32, 256
ks = [int(x) for x in a.ks.split(",")]
precisions = [int(x) for x in a.precisions.split(",")]
base = pkg.synth_sift(1_000_000, seed=20251205)
q = pkg.synth_sift(NB * B, seed=20251206)
vr, off, r2o, cents, it = pkg.ivf_build(base, 1024, max_iter=20, seed=42)
dev = torch.device("cuda", 0)
qd = torch.from_numpy(q).to(dev)
st = torch.cuda.current_stream().cuda_stream
with pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o) as ivf:
    for precision in precisions:
        ivf.set_precision(precision)
        for k in ks:
            o_i = torch.zeros((NB * B, k), dtype=torch.int32, device=dev)
            o_d = torch.zeros((NB * B, k), dtype=torch.float32, device=dev)
            call = lambda: ivf.search_dev_multi(qd.data_ptr(), NB, B, k, a.nprobe, o_i.data_ptr(), o_d.data_ptr(), st)
            if a.stats:
                if k <= 16:
                    continue
                call()
                torch.cuda.synchronize()
                cand, most, exact, ovf = ivf.widek_stats(reset=True)
                ranked = NB * B - exact
                print(f"precision {precision} k {k} nprobe {a.nprobe}: candidates per query mean {cand / max(ranked, 1):.1f} "
                      f"max {most}, ranked exactly {exact} of {NB * B} ({100.0 * exact / (NB * B):.2f} %), overflowed groups {ovf}",
                      flush=True)
                continue
            call()
            call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(6):
                call()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 6
            print(f"precision {precision} k {k} nprobe {a.nprobe}: {us:.1f} us per call of {NB * B} queries = "
                  f"{NB * B / us:.3f} M QPS", flush=True)
    if a.stats and a.recall_queries > 0:
        nq = a.recall_queries
        qr = pkg.synth_sift(nq, seed=20251207)
        exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "vsearch_bf")
        with tempfile.TemporaryDirectory() as tmp:
            bf, qf, gt = os.path.join(tmp, "base.fvecs"), os.path.join(tmp, "q.fvecs"), os.path.join(tmp, "gt.ivecs")
            pkg.write_fvecs(bf, base)
            pkg.write_fvecs(qf, qr)
            subprocess.run([exe, "--groundtruth", bf, qf, gt], check=True, capture_output=True, timeout=600)
            truth = pkg.read_ivecs(gt)
        for precision in precisions:
            ivf.set_precision(precision)
            ids, _, total = ivf.searchBatch(qr, nq, 100, a.nprobe)
            rec = np.mean([len(np.intersect1d(ids[i], truth[i])) / 100.0 for i in range(nq)])
            print(f"precision {precision}: recall@100 {rec:.4f} over {nq} queries (nprobe {a.nprobe}), "
                  f"{total / nq:.0f} rows scanned per query", flush=True)
