"""List-major IVF at a general dimension against exact brute force on the same rows: device time per 1024 queries.

    python scripts/ivf_nd_bench.py [--dims 96,384,768] [--rows 1000000] [--nlist 1024] [--nprobe 8,32] [--groups 4] [--reps 5]
                                   [--build ITERS] [--u8] [--widek K] [--metric ip [--k 10,100]]

Data: synth_sift rows (integer valued) at every dimension, nlist sampled rows as centroids, every row assigned to its
nearest centroid through the library's own brute force (a timing index, not a trained one).  Queries: `groups` groups of
1024 distinct synth_sift rows of another seed (32 batches of 32), k = 10.  The yardstick is BruteForceIndex on the same rows
(vs_bf_create_nd, fp32 rows, search_dev_multi), alternated with the IVF calls in the same process; a timed window is all
groups of one path between two device events, reported per 1024 queries, every repeat listed.  recall@10 is IVF against
that exact result.  bytes_ratio is the expectation to compare against: brute force reads N rows per 32 queries, the list
scan group_q * nprobe / 16 blocks of N / nlist rows.  Each dimension runs in a process of its own; one JSON line per
measurement.

--build ITERS trains the index with the library's builder instead (ivf_kmeans: vs_ivf_build_nd, k-means++ seeds, ITERS Lloyd
iterations at tol = 0, seed 42) and prints one more JSON line: the build's wall time, the device time of one assignment
pass (vs_ivf_build_last_assign_ms) and the iterations done; after the brute-force timing, a line that sets the assignment
pass against its yardstick, nlist / 32 x the per-batch time of the brute-force general scan on the same rows.  At dim 128
it prints the wall time of the specialised builder and of the general one (VSEARCH_BUILD_ND_FORCE=1), alternated, and stops.

--u8 takes the rows as uint8 (synth_sift rows are byte valued) and alternates three paths on them in one process: the
byte index (IVFIndex.from_u8: vs_ivf_create_nd_u8, paths ivf_u8_nprobeP), the vs_ivf_create index on the rows as float
(ivf_nprobeP, the yardstick) and exact brute force.  Both indexes must return the same ids and distance bits.  After the
end-to-end windows it times the list-scan launches alone (vs_prof_read(.., 1): the fp32 scan on one index, the fp32 scan
on an empty plan plus the byte scan on the other), again alternated, and prints the byte index's pair counts
(vs_ivf_nd_u8_stats: pairs planned on bytes, pairs planned on fp32).

--widek K (17 <= K <= 128) times the wide-k call of the general index (IVFIndex.search_topk_dev_multi at k = K, paths
ivf_kK_nprobeP) against two references alternated in the same process: the same index at k = 10 (ivf_k10_nprobeP) and exact
wide-k brute force on the same rows (bf_kK: BruteForceIndex.search_topk_dev_multi at k = K).  It also prints recall@K
against that exact result, the three counters of vs_ivf_nd_widek_stats for one pass over the queries, and the share of
(query, probe) pairs the rescan takes -- recomputed on the host in float64 for the first 64 queries (a pair is rescanned
when the 16th best distance of its list is at or under the K-th smallest of the query's per-list top-16s).

--metric ip times inner-product search through the per-call metric (IVFIndex.search_metric_dev_multi) against squared L2
through the same call on the same index in the same process, the L2 leg twice (paths l2_a and l2_b: their spread is the
noise an inner-product difference has to exceed), for every k of --k and every nprobe; with --u8 also the byte index
under inner product (ip_u8: the pairs on the byte rows for k <= 16) beside the fp32 index (ip).  Per path: us per 1024
queries between two device events and the list-scan launches alone (vs_prof_read(.., 1)).  recall@10 is inner-product IVF
against exact inner-product brute force on the same rows (BruteForceIndex(metric=METRIC_IP)).  A "probe_spread" line per
metric and nprobe says how many distinct lists a group of 1024 queries probes and how many rows a query's lists hold
(host, float64): on rows that are not normalised the inner-product probes of all queries fall on the same few lists.
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
GROUP_Q, B, K = 1024, 32, 10


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    base = pkg.synth_sift(a.rows, seed=1, dim=dim)
    q = pkg.synth_sift(a.groups * GROUP_Q, seed=2, dim=dim)
    if a.build and dim == 128:
        build_128(a, pkg, base)
        return
    assign_pass_ms = None
    if a.build:
        assign, cents, assign_pass_ms = build(a, pkg, base, dim)
    else:
        assign, cents = sampled_rows(a, pkg, base, dev, st)
    vr, off, r2o = pkg.ivf_layout_from_assignment(base, assign, a.nlist)
    if a.widek:
        search_widek(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st)
        return
    if a.metric == "ip":
        search_ip(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st)
        return
    search(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st, assign_pass_ms)


def build(a, pkg, base, dim):
    """the trained index: k-means through the library's builder"""
    t0 = time.perf_counter()
    cents, assign, iters = pkg.ivf_kmeans(base, a.nlist, a.build, 0.0, 42)
    wall = time.perf_counter() - t0
    assign_pass_ms = round(float(pkg.lib().vs_ivf_build_last_assign_ms()), 3)
    print(json.dumps({"what": "build", "dim": dim, "rows": a.rows, "nlist": a.nlist, "max_iter": a.build, "iters_done": iters,
                      "build_wall_s": round(wall, 3), "assign_pass_ms": assign_pass_ms}), flush=True)
    return assign, cents, assign_pass_ms


def build_128(a, pkg, base):
    """dim 128: the specialised builder (vs_ivf_build) and the general one (vs_ivf_build_nd under the toggle), alternated"""
    import ctypes as C
    n = base.shape[0]
    cents = np.empty((a.nlist, 128), dtype=np.float32)
    assign = np.empty(n, dtype=np.int32)
    it = C.c_int(0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    out = {"specialised": [], "general": []}
    keep = {}
    for _ in range(2):
        for name in ("specialised", "general"):
            if name == "general":
                os.environ["VSEARCH_BUILD_ND_FORCE"] = "1"
            try:
                t0 = time.perf_counter()
                rc = pkg.lib().vs_ivf_build_nd(p(base), n, 128, a.nlist, a.build, 0.0, 42, 0, p(cents), p(assign), C.byref(it))
                wall = time.perf_counter() - t0
            finally:
                os.environ.pop("VSEARCH_BUILD_ND_FORCE", None)
            if rc:
                raise RuntimeError(pkg.lib().vs_last_error().decode())
            out[name].append({"build_wall_s": round(wall, 3), "assign_pass_ms": round(float(pkg.lib().vs_ivf_build_last_assign_ms()), 3),
                              "iters_done": it.value})
            keep.setdefault(name, (cents.copy(), assign.copy()))
    same = bool(np.array_equal(keep["specialised"][0].view(np.uint32), keep["general"][0].view(np.uint32)) and
                np.array_equal(keep["specialised"][1], keep["general"][1]))
    print(json.dumps({"what": "build_128", "rows": n, "nlist": a.nlist, "max_iter": a.build, **out, "same_bits": same}), flush=True)


def sampled_rows(a, pkg, base, dev, st):
    """the timing index: nlist sampled rows as centroids, every row assigned to its nearest one"""
    import torch
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
    return assign, cents


def search(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st, assign_pass_ms):
    import torch
    sizes = np.diff(off)
    print(json.dumps({"what": "index", "dim": dim, "rows": a.rows, "nlist": a.nlist, "list_min": int(sizes.min()),
                      "list_mean": float(sizes.mean()), "list_max": int(sizes.max())}), flush=True)

    qd = torch.from_numpy(q).to(dev)
    nbg = GROUP_Q // B
    nprobes = [int(x) for x in a.nprobe.split(",")]
    import contextlib
    with contextlib.ExitStack() as stack:
        bf = stack.enter_context(pkg.BruteForceIndex(base))
        ivf = stack.enter_context(pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o))
        ivf8 = None
        if a.u8:
            rows_u8 = vr.astype(np.uint8)
            assert np.array_equal(rows_u8.astype(np.float32), vr), "--u8 needs byte-valued rows"
            ivf8 = stack.enter_context(pkg.IVFIndex.from_u8(rows_u8, cents, off, r2o))
            del rows_u8
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

        def run_ivf(nprobe, index=ivf):
            for g in range(a.groups):
                o = g * GROUP_Q
                index.search_dev_multi(qd[o].data_ptr(), nbg, B, K, nprobe, ii[o].data_ptr(), idd[o].data_ptr(), st)

        def timed(f, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(*args)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.groups  # us per 1024 queries

        paths = [("bf", run_bf, ())] + [(f"ivf_nprobe{p}", run_ivf, (p,)) for p in nprobes]
        if a.u8:
            paths += [(f"ivf_u8_nprobe{p}", run_ivf, (p, ivf8)) for p in nprobes]
        recall, results = {}, {}
        for name, f, args in paths:  # warm-up of every path, and the recall of the IVF ones
            f(*args)
            f(*args)
            torch.cuda.synchronize()
            if name == "bf":
                exact = bi[:, :K].cpu().numpy()
            else:
                got = ii.cpu().numpy()
                recall[name] = float(np.mean([len(set(got[i]) & set(exact[i])) / K for i in range(len(exact))]))
                results[name] = (got, idd.cpu().numpy().view(np.int32).copy())
        if a.u8:  # faster and different is not faster: the byte index returns the fp32 index's ids and distance bits
            for p in nprobes:
                x, y = results[f"ivf_nprobe{p}"], results[f"ivf_u8_nprobe{p}"]
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), f"byte index differs at nprobe {p}"
        us = {name: [] for name, _, _ in paths}
        for _ in range(a.reps):
            for name, f, args in paths:
                us[name].append(timed(f, *args))
        med = {n: sorted(v)[len(v) // 2] for n, v in us.items()}
        if assign_pass_ms is not None:  # the assignment pass against nlist / 32 passes of the brute-force scan over the same rows
            yard = med["bf"] / (GROUP_Q // B) * (a.nlist / B) / 1e3
            print(json.dumps({"what": "assign_vs_yardstick", "dim": dim, "rows": a.rows, "nlist": a.nlist, "assign_pass_ms": assign_pass_ms,
                              "bf_us_per_batch": round(med["bf"] / (GROUP_Q // B), 2), "yardstick_ms": round(yard, 3),
                              "ratio": round(assign_pass_ms / yard, 3)}), flush=True)
        for name, _, args in paths:
            rec = {"what": "us_per_1024_queries", "path": name, "dim": dim, "rows": a.rows, "nlist": a.nlist, "k": K,
                   "us": [round(u, 1) for u in us[name]], "median_us": round(med[name], 1)}
            if args:
                rec["recall_at_10"] = round(recall[name], 4)
                rec["speedup_vs_bf"] = round(med["bf"] / med[name], 2)
                rec["bytes_ratio"] = round((GROUP_Q / B) / (GROUP_Q * args[0] / 16.0 / a.nlist), 2)
            print(json.dumps(rec), flush=True)
        if a.u8:  # the list-scan launches alone (vs_prof_read window 1), the two indexes alternated
            scan = {(name, p): [] for name in ("fp32", "u8") for p in nprobes}
            for _ in range(a.reps):
                for p in nprobes:
                    for name, index in (("fp32", ivf), ("u8", ivf8)):
                        index.prof_enable(True)
                        run_ivf(p, index)
                        torch.cuda.synchronize()
                        ms, n = index.prof_read(1)
                        index.prof_enable(False)
                        assert n == a.groups
                        scan[(name, p)].append(ms / n)
            for p in nprobes:
                ivf8.nd_u8_stats(reset=True)
                run_ivf(p, ivf8)
                on_bytes, on_fp32 = ivf8.nd_u8_stats()
                f, b = sorted(scan[("fp32", p)]), sorted(scan[("u8", p)])
                print(json.dumps({"what": "list_scan_ms_per_group", "dim": dim, "nprobe": p, "fp32_index": [round(x, 3) for x in scan[("fp32", p)]],
                                  "u8_index": [round(x, 3) for x in scan[("u8", p)]], "fp32_median": round(f[len(f) // 2], 3),
                                  "u8_median": round(b[len(b) // 2], 3), "ratio": round(f[len(f) // 2] / b[len(b) // 2], 2),
                                  "pairs_on_bytes": on_bytes, "pairs_on_fp32": on_fp32}), flush=True)


def rescan_share(vr, off, cents, q, k, nprobe):
    """share of the (query, probe) pairs with rows that the wide-k rescan takes, recomputed in float64"""
    c64 = cents.astype(np.float64)
    cn = (c64 * c64).sum(1)
    taken = pairs = 0
    for x in q.astype(np.float64):
        probes = np.argsort(cn - 2 * c64 @ x, kind="stable")[:nprobe]
        tops = []
        for c in probes:
            rows = vr[off[c]:off[c + 1]].astype(np.float64)
            if len(rows):
                tops.append(np.sort(((rows - x) ** 2).sum(1))[:16])
        if not tops:
            continue
        every = np.sort(np.concatenate(tops))
        tau = every[k - 1] if len(every) >= k else np.inf
        pairs += len(tops)
        taken += sum(1 for t in tops if len(t) == 16 and t[15] <= tau)
    return taken / max(pairs, 1)


def search_widek(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st):
    import torch
    KW = a.widek
    sizes = np.diff(off)
    print(json.dumps({"what": "index", "dim": dim, "rows": a.rows, "nlist": a.nlist, "list_min": int(sizes.min()),
                      "list_mean": float(sizes.mean()), "list_max": int(sizes.max())}), flush=True)
    qd = torch.from_numpy(q).to(dev)
    nq, nbg = a.groups * GROUP_Q, GROUP_Q // B
    nprobes = [int(x) for x in a.nprobe.split(",")]
    share = {p: rescan_share(vr, off, cents, q[:64], KW, p) for p in nprobes}
    with pkg.BruteForceIndex(base) as bf, pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off,
                                                      reorder_to_original=r2o) as ivf:
        bf.set_precision(1)
        bi = torch.empty((nq, KW + 1), dtype=torch.int32, device=dev)
        bd = torch.empty((nq, KW + 1), dtype=torch.float32, device=dev)
        bfl = torch.empty((nq,), dtype=torch.int32, device=dev)
        wi = torch.empty((nq, KW), dtype=torch.int32, device=dev)
        wd = torch.empty((nq, KW), dtype=torch.float32, device=dev)
        ii = torch.empty((nq, K), dtype=torch.int32, device=dev)
        idd = torch.empty((nq, K), dtype=torch.float32, device=dev)

        def run_bf():
            for g in range(a.groups):
                o = g * GROUP_Q
                bf.search_topk_dev_multi(qd[o].data_ptr(), nbg, B, KW, bi[o].data_ptr(), bd[o].data_ptr(), bfl[o].data_ptr(), st)

        def run_k10(nprobe):
            for g in range(a.groups):
                o = g * GROUP_Q
                ivf.search_dev_multi(qd[o].data_ptr(), nbg, B, K, nprobe, ii[o].data_ptr(), idd[o].data_ptr(), st)

        def run_wide(nprobe):
            for g in range(a.groups):
                o = g * GROUP_Q
                ivf.search_topk_dev_multi(qd[o].data_ptr(), nbg, B, KW, nprobe, wi[o].data_ptr(), wd[o].data_ptr(), st)

        def timed(f, *args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(*args)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.groups  # us per 1024 queries

        paths = [(f"bf_k{KW}", run_bf, ())]
        for p in nprobes:
            paths += [(f"ivf_k{K}_nprobe{p}", run_k10, (p,)), (f"ivf_k{KW}_nprobe{p}", run_wide, (p,))]
        recall, stats = {}, {}
        for name, f, args in paths:  # warm-up of every path; recall and counters of the wide ones
            f(*args)
            torch.cuda.synchronize()
            if f is run_wide:
                ivf.nd_widek_stats(reset=True)
            f(*args)
            torch.cuda.synchronize()
            if f is run_bf:
                exact = bi[:, :KW].cpu().numpy()
            elif f is run_wide:
                stats[name] = ivf.nd_widek_stats(reset=True)
                got = wi.cpu().numpy()
                recall[name] = float(np.mean([len(set(got[i]) & set(exact[i])) / KW for i in range(nq)]))
        us = {name: [] for name, _, _ in paths}
        for _ in range(a.reps):
            for name, f, args in paths:
                us[name].append(timed(f, *args))
        med = {n: sorted(v)[len(v) // 2] for n, v in us.items()}
        for name, f, args in paths:
            rec = {"what": "us_per_1024_queries", "path": name, "dim": dim, "rows": a.rows, "nlist": a.nlist,
                   "k": K if f is run_k10 else KW, "us": [round(u, 1) for u in us[name]], "median_us": round(med[name], 1)}
            if f is run_wide:
                p = args[0]
                rec[f"recall_at_{KW}"] = round(recall[name], 4)
                rec["ratio_to_k10"] = round(med[name] / med[f"ivf_k{K}_nprobe{p}"], 2)
                rec["speedup_vs_bf_wide"] = round(med[f"bf_k{KW}"] / med[name], 2)
                rec["widek_stats"] = list(stats[name])
                rec["candidates_per_query"] = round(stats[name][0] / max(nq - stats[name][2], 1), 1)
                rec["rescan_share_first_64_queries"] = round(share[p], 4)
                rec["rescan_share_expected"] = round(KW / (16.0 * p), 4)
            print(json.dumps(rec), flush=True)


def search_ip(a, pkg, dim, base, q, vr, off, r2o, cents, dev, st):
    import contextlib
    import torch
    sizes = np.diff(off)
    print(json.dumps({"what": "index", "dim": dim, "rows": a.rows, "nlist": a.nlist, "list_min": int(sizes.min()),
                      "list_mean": float(sizes.mean()), "list_max": int(sizes.max())}), flush=True)
    qd = torch.from_numpy(q).to(dev)
    nq, nbg = a.groups * GROUP_Q, GROUP_Q // B
    nprobes = [int(x) for x in a.nprobe.split(",")]
    ks = [int(x) for x in a.k.split(",")]
    # how the probes spread, recomputed on the host in float64: the list-major scan reads a probed list once per 16 of the
    # group's queries that probe it, so the fewer distinct lists a group of 1024 queries probes, the more of its reads hit
    c64, q64 = cents.astype(np.float64), q.astype(np.float64)
    dots = q64 @ c64.T
    for name, sc in (("l2", (c64 * c64).sum(1)[None, :] - 2 * dots), ("ip", -dots)):
        for p in nprobes:
            pr = np.argpartition(sc, p - 1, axis=1)[:, :p]
            distinct = [len(np.unique(pr[g * GROUP_Q:(g + 1) * GROUP_Q])) for g in range(a.groups)]
            print(json.dumps({"what": "probe_spread", "metric": name, "dim": dim, "nprobe": p, "distinct_lists_per_group": distinct,
                              "rows_per_query": round(float(sizes[pr].sum()) / nq, 1)}), flush=True)
    del c64, q64, dots
    with contextlib.ExitStack() as stack:
        bf = stack.enter_context(pkg.BruteForceIndex(base, metric=pkg.METRIC_IP))
        bf.set_precision(1)
        bi = torch.empty((nq, K + 1), dtype=torch.int32, device=dev)
        bd = torch.empty((nq, K + 1), dtype=torch.float32, device=dev)
        bfl = torch.empty((nq,), dtype=torch.int32, device=dev)
        for g in range(a.groups):
            o = g * GROUP_Q
            bf.search_dev_multi(qd[o].data_ptr(), nbg, B, K, bi[o].data_ptr(), bd[o].data_ptr(), bfl[o].data_ptr(), st)
        torch.cuda.synchronize()
        exact = bi[:, :K].cpu().numpy()
        bf.close()
        del bi, bd, bfl
        ivf = stack.enter_context(pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o))
        ivf8 = None
        if a.u8:
            rows_u8 = vr.astype(np.uint8)
            assert np.array_equal(rows_u8.astype(np.float32), vr), "--u8 needs byte-valued rows"
            ivf8 = stack.enter_context(pkg.IVFIndex.from_u8(rows_u8, cents, off, r2o))
            del rows_u8
        del vr
        for k in ks:
            oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)

            def run(index, metric, nprobe):
                for g in range(a.groups):
                    o = g * GROUP_Q
                    index.search_metric_dev_multi(qd[o].data_ptr(), nbg, B, k, nprobe, metric, oi[o].data_ptr(), od[o].data_ptr(), st)

            def timed(*args):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(*args)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.groups  # us per 1024 queries

            for p in nprobes:
                paths = [("l2_a", ivf, pkg.METRIC_L2), ("ip", ivf, pkg.METRIC_IP), ("l2_b", ivf, pkg.METRIC_L2)]
                if ivf8 is not None:
                    paths.append(("ip_u8", ivf8, pkg.METRIC_IP))
                recall, results, pairs = {}, {}, None
                for name, index, metric in paths:  # warm-up of every path; recall of the inner-product ones
                    run(index, metric, p)
                    if name == "ip_u8":
                        index.nd_u8_stats(reset=True)
                    run(index, metric, p)
                    torch.cuda.synchronize()
                    if name == "ip_u8":
                        pairs = index.nd_u8_stats()
                    if metric == pkg.METRIC_IP:
                        got = oi.cpu().numpy()
                        recall[name] = float(np.mean([len(set(got[i, :K]) & set(exact[i])) / K for i in range(nq)]))
                        results[name] = (got, od.cpu().numpy().view(np.int32).copy())
                if ivf8 is not None:  # the byte index returns the fp32 index's ids and score bits
                    x, y = results["ip"], results["ip_u8"]
                    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), f"byte index differs at k {k}, nprobe {p}"
                us = {name: [] for name, _, _ in paths}
                scan = {name: [] for name, _, _ in paths}
                for _ in range(a.reps):
                    for name, index, metric in paths:
                        us[name].append(timed(index, metric, p))
                for _ in range(a.reps):  # the list-scan launches alone
                    for name, index, metric in paths:
                        index.prof_enable(True)
                        run(index, metric, p)
                        torch.cuda.synchronize()
                        ms, n = index.prof_read(1)
                        index.prof_enable(False)
                        scan[name].append(ms / max(n, 1) * 1e3)
                med = lambda v: sorted(v)[len(v) // 2]
                l2 = 0.5 * (med(us["l2_a"]) + med(us["l2_b"]))
                l2s = 0.5 * (med(scan["l2_a"]) + med(scan["l2_b"]))
                for name, _, metric in paths:
                    rec = {"what": "ip_vs_l2", "path": name, "dim": dim, "rows": a.rows, "nlist": a.nlist, "k": k, "nprobe": p,
                           "us_per_1024": [round(u, 1) for u in us[name]], "median_us": round(med(us[name]), 1),
                           "scan_us_per_group": [round(u, 1) for u in scan[name]], "scan_median_us": round(med(scan[name]), 1)}
                    if metric == pkg.METRIC_IP:
                        rec["recall_at_10"] = round(recall[name], 4)
                        rec["ratio_to_l2"] = round(med(us[name]) / l2, 3)
                        rec["scan_ratio_to_l2"] = round(med(scan[name]) / l2s, 3)
                    if name == "ip_u8":
                        rec["pairs_on_bytes"], rec["pairs_on_fp32"] = pairs
                        rec["scan_ratio_to_ip_fp32"] = round(med(scan[name]) / med(scan["ip"]), 3)
                    if name == "l2_b":
                        rec["l2_spread"] = round(abs(med(us["l2_a"]) - med(us["l2_b"])) / l2, 4)
                        rec["l2_scan_spread"] = round(abs(med(scan["l2_a"]) - med(scan["l2_b"])) / l2s, 4)
                    print(json.dumps(rec), flush=True)
            del oi, od


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,384,768")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", default="8,32")
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build", type=int, default=0, metavar="ITERS", help="train the index with the library's builder")
    ap.add_argument("--u8", action="store_true", help="rows as uint8: the byte index beside the vs_ivf_create index and brute force")
    ap.add_argument("--widek", type=int, default=0, metavar="K", help="time the wide-k call (17 <= K <= 128) against k = 10 and exact wide-k brute force")
    ap.add_argument("--metric", default="l2", choices=["l2", "ip"], help="ip: inner product against L2 through the per-call metric")
    ap.add_argument("--k", default="10,100", help="the k values of the --metric ip leg")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(a, a.one)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--nlist", str(a.nlist), "--nprobe", a.nprobe,
           "--groups", str(a.groups), "--reps", str(a.reps), "--build", str(a.build)] + (["--u8"] if a.u8 else []) + ["--widek", str(a.widek)]
    cmd += ["--metric", a.metric, "--k", a.k]
    for dim in [int(x) for x in a.dims.split(",")]:
        r = subprocess.run(cmd + ["--one", str(dim)], timeout=900)
        if r.returncode != 0:  # a failed or faulted step ends the run: nothing more is started on the GPU
            sys.exit(r.returncode if r.returncode > 0 else 1)


if __name__ == "__main__":
    main()
