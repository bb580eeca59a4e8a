"""The int16 cosine runner at N = 1 M rows, B = 32: device time per batch of vs_i16_execute_dev (quantiser + score matrix)
and of vs_i16_search_dev (quantiser + fused top-k scan + merge, k = 10), by HIP events, beside the fp32 general scan under
inner product (BruteForceIndex, precision 1) and the byte scan (BruteForceIndex.from_u8(metric=METRIC_IP), precision 2) on
the same rows, in the same process, alternated.  One JSON line per leg with every repeat, then one with the medians and
ratios; hbm_frac is the leg's row bytes over its time as a share of the HBM peak (i16: 2 N dim_h bytes, dim_h = dim rounded
up to 32 values; fp32: 4 N dim_p; bytes: N dim_b).

    python scripts/i16_bench.py [--dims 96,128,384,768,2048] [--rows 1000000] [--reps 7] > profiles/i16_bench.txt

Each dimension runs in a process of its own; at 128 the process runs under VSEARCH_ND_FORCE=1, so that the fp32 leg is the
general scan there too and not the specialised 128-d index.  The rows are integers in [0, 64) (so that the byte index
accepts them); the queries likewise.  The three indexes rank by different scores (cosine / inner product), so only times
are compared here; tests/test_gpu_i16.py checks the results.

    python scripts/i16_bench.py --wide-k [K] [--dims 96,384,768,2048] > profiles/i16_wide_k_bench.txt

The wide-k leg (K = 100 unless given): vs_i16_search_topk_dev at k = K beside the fused k = 10 call of the same runner,
same settings (16 batches of 32 per call, HIP events, alternated repeats, medians), on gaussian rows; then the candidates per
query and the fallback count from vs_i16_wide_stats, and recall@K of the int16 ranking against
BruteForceIndex(..., METRIC_IP).search_topk at fp32 on the same L2-normalised rows.  tests/test_gpu_i16_wide_k.py checks the
results themselves.
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


def _data(rows, dim, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=np.uint8)
    step = max(1, (1 << 26) // dim)
    for r0 in range(0, rows, step):
        out[r0:r0 + step] = rng.integers(0, 64, size=(min(step, rows - r0), dim), dtype=np.uint8)
    return out


def one(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    nb, B, k = 16, 32, 10
    base_u8 = _data(a.rows, dim, 1)
    base = base_u8.astype(np.float32)
    with pkg.I16Runner(base) as r16, pkg.BruteForceIndex(base, metric=pkg.METRIC_IP) as f32, \
            pkg.BruteForceIndex.from_u8(base_u8, metric=pkg.METRIC_IP) as u8:
        del base, base_u8
        f32.set_precision(1)
        u8.set_precision(2)
        dev = torch.device("cuda:0")
        qd = torch.from_numpy(_data(nb * B, dim, 2).astype(np.float32)).to(dev)
        ids = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
        top = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
        dist = torch.empty((nb * B, k + 1), dtype=torch.float32, device=dev)
        fl = torch.empty((nb * B,), dtype=torch.int32, device=dev)
        mat = torch.empty((B, a.rows), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def i16_execute():
            for b in range(nb):
                r16.execute_dev(qd.data_ptr() + 4 * b * B * dim, B, mat.data_ptr(), a.rows, st)

        legs = {
            "i16_execute": i16_execute,
            "i16_search": lambda: r16.search_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), st),
            "ip_fp32": lambda: f32.search_dev_multi(qd.data_ptr(), nb, B, k, ids.data_ptr(), dist.data_ptr(), fl.data_ptr(), st),
            "ip_u8": lambda: u8.search_dev_multi(qd.data_ptr(), nb, B, k, ids.data_ptr(), dist.data_ptr(), fl.data_ptr(), st),
        }

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / nb  # us per batch

        for call in legs.values():  # warm-up of every kernel the timed window uses
            for _ in range(2):
                call()
            torch.cuda.synchronize()
        assert not bool((fl == 2).any()), "a batch was refused by the byte scan"
        us = {leg: [] for leg in legs}
        for _ in range(a.reps):  # alternated: one repeat of every leg, then the next repeat
            for leg, call in legs.items():
                us[leg].append(timed(call))
        dim_h, dim_p, dim_b = (dim + 31) // 32 * 32, (dim + 15) // 16 * 16, (dim + 63) // 64 * 64
        row_bytes = {"i16_execute": 2 * dim_h, "i16_search": 2 * dim_h, "ip_fp32": 4 * dim_p, "ip_u8": dim_b}
        for leg in legs:
            frac = [a.rows * float(row_bytes[leg]) / (u * 1e-6) / 1e9 / HBM_PEAK_GBS for u in us[leg]]
            print(json.dumps({"what": "us_per_batch", "leg": leg, "dim": dim, "rows": a.rows, "B": B, "k": k, "row_bytes": row_bytes[leg],
                              "us_per_batch": [round(u, 2) for u in us[leg]], "hbm_frac": [round(f, 4) for f in frac]}), flush=True)
        med = {leg: sorted(v)[len(v) // 2] for leg, v in us.items()}
        print(json.dumps({"what": "i16_vs_others", "dim": dim, "rows": a.rows, **{"median_us_" + leg: round(m, 2) for leg, m in med.items()},
                          "fp32_over_i16_search": round(med["ip_fp32"] / med["i16_search"], 3),
                          "u8_over_i16_search": round(med["ip_u8"] / med["i16_search"], 3),
                          # the score matrix itself is 4 B N bytes written per batch, on top of the rows read
                          "execute_write_bytes": 4 * B * a.rows}), flush=True)


def _unit_rows(rows, dim, seed):
    """Gaussian rows, L2-normalised, generated in chunks."""
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=np.float32)
    step = max(1, (1 << 25) // dim)
    for r0 in range(0, rows, step):
        x = rng.standard_normal((min(step, rows - r0), dim), dtype=np.float32)
        out[r0:r0 + step] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def one_wide(a, dim):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    nb, B, k, kw = 16, 32, 10, a.wide_k
    base = _unit_rows(a.rows, dim, 1)
    q = _unit_rows(nb * B, dim, 2)
    with pkg.I16Runner(base) as r16:
        dev = torch.device("cuda:0")
        qd = torch.from_numpy(q).to(dev)
        ids = torch.empty((nb * B, k), dtype=torch.int32, device=dev)
        top = torch.empty((nb * B, k), dtype=torch.int32, device=dev)
        wids = torch.empty((nb * B, kw), dtype=torch.int32, device=dev)
        wtop = torch.empty((nb * B, kw), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        legs = {
            "i16_search": lambda: r16.search_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), st),
            "i16_search_topk": lambda: r16.search_topk_dev(qd.data_ptr(), nb, B, kw, wids.data_ptr(), wtop.data_ptr(), st),
        }

        def timed(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / nb  # us per batch

        for call in legs.values():
            for _ in range(2):
                call()
            torch.cuda.synchronize()
        r16.wide_stats(reset=True)
        us = {leg: [] for leg in legs}
        for _ in range(a.reps):
            for leg, call in legs.items():
                us[leg].append(timed(call))
        ranked, cand_max, dense, whole = r16.wide_stats(reset=True)
        for leg in legs:
            print(json.dumps({"what": "us_per_batch", "leg": leg, "dim": dim, "rows": a.rows, "B": B, "k": kw if leg == "i16_search_topk" else k,
                              "us_per_batch": [round(u, 2) for u in us[leg]]}), flush=True)
        med = {leg: sorted(v)[len(v) // 2] for leg, v in us.items()}
        # candidates per query: the host call on the same queries, whose lists the counters describe
        wi, _ = r16.search_topk(q, kw)
        assert np.array_equal(wi, wids.cpu().numpy())
        _, cand_max1, dense1, _ = r16.wide_stats(reset=True)
    if a.profile_only:
        return
    with pkg.BruteForceIndex(base, metric=pkg.METRIC_IP) as f32:
        f32.set_precision(1)
        fi, _ = f32.search_topk(q, kw)
    recall = float(np.mean([len(np.intersect1d(wi[i], fi[i])) / kw for i in range(len(q))]))
    sg, stride, cap = pkg.i16_wide_plan(a.rows, kw)
    print(json.dumps({"what": "wide_k", "dim": dim, "rows": a.rows, "k": kw, "sample_groups": sg, "stride": stride, "cap": cap,
                      "median_us_i16_search_k10": round(med["i16_search"], 2), "median_us_i16_search_topk": round(med["i16_search_topk"], 2),
                      "topk_over_k10": round(med["i16_search_topk"] / med["i16_search"], 3),
                      "queries_ranked_from_lists": ranked, "queries_dense_fallback": dense + dense1, "queries_whole_sample": whole,
                      "candidates_max": max(cand_max, cand_max1), "recall_at_k_vs_fp32_ip": round(recall, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128,384,768,2048")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--wide-k", type=int, nargs="?", const=100, default=0, help="the wide-k leg instead: k of vs_i16_search_topk_dev (17..128)")
    ap.add_argument("--profile-only", action="store_true", help="wide-k leg: stop after the timed calls (for a run under a profiler)")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one_wide(a, a.one) if a.wide_k else one(a, a.one)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--reps", str(a.reps)]
    if a.wide_k:
        cmd += ["--wide-k", str(a.wide_k)] + (["--profile-only"] if a.profile_only else [])
        if a.dims == ap.get_default("dims"):
            a.dims = "96,384,768,2048"
    for dim in [int(x) for x in a.dims.split(",")]:
        env = dict(os.environ)
        if dim == 128:  # the fp32 leg is the general scan at every dimension (vs_bf_create's comparison toggle, read at load)
            env["VSEARCH_ND_FORCE"] = "1"
        r = subprocess.run(cmd + ["--one", str(dim)], timeout=600, env=env)
        if r.returncode != 0:  # a failed or faulted step ends the run: nothing more is started on the GPU
            sys.exit(r.returncode if r.returncode > 0 else 1)


if __name__ == "__main__":
    main()
