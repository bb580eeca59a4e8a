"""Wide-k brute force (k >= 16) on a general index made from uint8 rows, N = 1 M synth_sift rows: device time per batch of 32
queries of search_topk_dev_multi, timed back to back by HIP events, on the byte route (scan_nd_i8_wide_kernel)
against the same library under VSEARCH_ND_WIDE_U8=0 (the fp32 launches) in an alternated process with an index of its own.

    python scripts/nd_wide_u8_bench.py [--dims 96,128ip,384,768,2048] [--ks 16,100,128] [--rows 1000000] [--reps 5] [--rounds 1]
    python scripts/nd_wide_u8_bench.py --root <another checkout, built> --only off ...   # the same fp32 leg on another build

Legs of the default process (one index): `u8` the byte route; `prec1` precision 1 on the same index (the fp32 launches
alone); `mixed` precision 0 with one non-integer value in every batch (every batch is answered by the fp32 launches behind
idle byte launches: the cost of those).  Leg of the toggled process: `off`.  A dimension with the suffix `ip` is measured
under inner product.  Every repeat is listed; the summary line per (dim, k) has the medians, the spread (max - min) of each
leg and the rule's verdict: the byte route stays when its median beats `off` by more than the larger spread of the two.
Each process is one step with a time limit of its own; a failed step ends the run."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows_u8(pkg, rows, dim, seed):
    out = np.empty((rows, dim), dtype=np.uint8)
    step = max(1, (1 << 25) // dim)
    for r0 in range(0, rows, step):
        out[r0:r0 + step] = pkg.synth_sift(min(step, rows - r0), seed=seed, dim=dim, row_begin=r0)
    return out


def _sq(a):
    return int((a.astype(np.int64) ** 2).sum(1).max())


def worker(a):
    root = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, root)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dim, ip = int(a.one.rstrip("ip")), a.one.endswith("ip")
    nb, B = a.nb, 32
    base = _rows_u8(pkg, a.rows, dim, 1)
    q = _rows_u8(pkg, nb * B, dim, 2)
    shift = 0
    while _sq(base) + _sq(q) > 2 ** 24:  # the exactness rule must admit every batch: halve the values until it does
        base >>= 1
        q >>= 1
        shift += 1
    kw = {"metric": pkg.METRIC_IP} if ip else {}
    with pkg.BruteForceIndex.from_u8(base, **kw) as idx:
        del base
        dev = torch.device("cuda:0")
        qf = q.astype(np.float32)
        qd = torch.from_numpy(qf).to(dev)
        qf[::B, 0] += 0.5  # one value that is no byte in every batch
        qmix = torch.from_numpy(qf).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        has_stats = hasattr(idx, "wide_stats")
        legs = ("off",) if a.leg == "off" else ("u8", "prec1", "mixed")
        for k in [int(x) for x in a.ks.split(",")]:
            oi = torch.empty((nb * B, k + 1), dtype=torch.int32, device=dev)
            od = torch.empty((nb * B, k + 1), dtype=torch.float32, device=dev)
            fl = torch.empty((nb * B,), dtype=torch.int32, device=dev)

            def timed(leg):
                idx.set_precision(1 if leg == "prec1" else 0)
                qq = qmix if leg == "mixed" else qd
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                idx.search_topk_dev_multi(qq.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / nb

            got = {}
            for leg in legs:  # warm-up, and what each leg's route was
                if has_stats:
                    idx.wide_stats(reset=True)
                timed(leg)
                timed(leg)
                if has_stats:
                    want = {"u8": (2 * nb, 0), "prec1": (0, 0), "mixed": (0, 2 * nb), "off": (0, 0)}[leg]
                    assert idx.wide_stats()[:2] == want, (leg, idx.wide_stats())
                assert not bool((fl == 2).any())
                got[leg] = (oi.clone(), od.clone())
            if "u8" in got:
                assert torch.equal(got["u8"][0], got["prec1"][0]) and torch.equal(got["u8"][1], got["prec1"][1]), "byte and fp32 results differ"
            us = {leg: [] for leg in legs}
            for _ in range(a.reps):
                for leg in legs:
                    us[leg].append(timed(leg))
            for leg in legs:
                print(json.dumps({"what": "wide_us_per_batch", "leg": leg, "dim": dim, "metric": "ip" if ip else "l2", "k": k,
                                  "rows": a.rows, "nb": nb, "B": B, "value_shift": shift, "build": a.tag,
                                  "us_per_batch": [round(u, 1) for u in us[leg]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128ip,384,768,2048")
    ap.add_argument("--ks", default="16,100,128")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="alternations of the two processes per dimension")
    ap.add_argument("--nb", type=int, default=8, help="batches per timed call")
    ap.add_argument("--only", choices=("both", "u8", "off"), default="both")
    ap.add_argument("--root", default="", help="load the package from this checkout instead (its `off` leg: another build's fp32 launches)")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--leg", default="u8", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        worker(a)
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--ks", a.ks, "--rows", str(a.rows), "--reps", str(a.reps), "--nb", str(a.nb),
           "--root", a.root, "--tag", a.tag]
    lines = []
    for dim in a.dims.split(","):
        for _ in range(a.rounds):
            for leg in ("u8", "off"):
                if a.only not in ("both", leg):
                    continue
                env = dict(os.environ)
                env.pop("VSEARCH_ND_WIDE_U8", None)
                if leg == "off":
                    env["VSEARCH_ND_WIDE_U8"] = "0"
                r = subprocess.run(cmd + ["--one", dim, "--leg", leg], env=env, timeout=600, capture_output=True, text=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if r.returncode != 0:  # a failed or faulted step ends the run: nothing more is started on the GPU
                    sys.stderr.write(r.stderr[-3000:])
                    sys.exit(r.returncode if r.returncode > 0 else 1)
                lines += [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    # medians and spreads per (dim, metric, k), repeats of every round pooled, and the rule
    keys = sorted({(x["dim"], x["metric"], x["k"]) for x in lines})
    for dim, metric, k in keys:
        s = {"what": "wide_summary", "dim": dim, "metric": metric, "k": k}
        for leg in ("u8", "off", "prec1", "mixed"):
            v = sorted(u for x in lines if (x["dim"], x["metric"], x["k"], x["leg"]) == (dim, metric, k, leg) for u in x["us_per_batch"])
            if v:
                s[leg + "_median_us"], s[leg + "_spread_us"] = v[len(v) // 2], round(v[-1] - v[0], 1)
        if "u8_median_us" in s and "off_median_us" in s:
            s["speedup"] = round(s["off_median_us"] / s["u8_median_us"], 3)
            s["stays_on_bytes"] = s["off_median_us"] - s["u8_median_us"] > max(s["u8_spread_us"], s["off_spread_us"])
        print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
