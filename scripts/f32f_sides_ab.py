#!/usr/bin/env python3
"""Settings of the bf16 prefilter sweep (scan_f32f_kernel) against each other, per launch size and shard size: every side
is a set of environment knobs (read when the library loads), optionally with a library of its own, run in alternated
processes, each timing search_dev_multi launch groups of 4, 8, 16 and 32 batches of 32 queries on a synthetic SIFT
shard with HIP events.  Prints every repeat: the figures DESIGN 4.2b chooses the defaults from.

    python3 scripts/f32f_sides_ab.py --sides "off:VSEARCH_F32F_PRIO=0 rule: on:VSEARCH_F32F_PRIO=4" \\
        [--repeats 3] [--rows 125000,250000,500000,1000000] [--batches 4,8,16,32]

A side is name:KEY=VALUE[,KEY=VALUE...]; the key LIB names another build of the library.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def worker(rows, batches):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    if os.environ.get("VSEARCH_AB_LIB"):
        pkg.LIB_PATH = os.path.abspath(os.environ["VSEARCH_AB_LIB"])
    dev = torch.device("cuda", 0)
    base = pkg.synth_sift(rows, seed=1)
    q = torch.from_numpy(pkg.synth_sift(1024, seed=2)).to(dev)
    sptr = torch.cuda.current_stream().cuda_stream
    out = {}
    with pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        for nb in batches:
            o_d = torch.zeros((nb * 32, 6), dtype=torch.float32, device=dev)
            o_i = torch.zeros((nb * 32, 6), dtype=torch.int32, device=dev)
            fl = torch.zeros((nb * 32,), dtype=torch.int32, device=dev)
            call = lambda: idx.search_dev_multi(q.data_ptr(), nb, 32, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), sptr)
            for _ in range(30):
                call()
            torch.cuda.synchronize()
            regions = []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    call()
                e1.record()
                torch.cuda.synchronize()
                regions.append(e0.elapsed_time(e1) * 1e3 / 50)
            out[nb] = round(statistics.median(regions), 2)
        launches, overflowed, _, _ = idx.filter_stats()
        assert launches > 0 and overflowed == 0, (launches, overflowed)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", default="off:VSEARCH_F32F_PRIO=0 rule: on:VSEARCH_F32F_PRIO=4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="125000,250000,500000,1000000")
    ap.add_argument("--batches", default="4,8,16,32")
    ap.add_argument("--worker", type=int, default=0)
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    if args.worker:
        return worker(args.worker, batches)
    sides = []
    for spec in args.sides.split():
        name, _, kv = spec.partition(":")
        env = dict(x.split("=", 1) for x in kv.split(",") if x)
        if "LIB" in env:
            env["VSEARCH_AB_LIB"] = env.pop("LIB")
        sides.append((name, env))
    for rows in (int(x) for x in args.rows.split(",")):
        res = {name: [] for name, _ in sides}
        for rep in range(args.repeats):
            for name, senv in sides:
                env = dict(os.environ, VSEARCH_SEED_MIN="1", **senv)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(rows), "--batches", args.batches],
                                   env=env, check=True, capture_output=True, text=True, timeout=300)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
                res[name].append({int(k): v for k, v in json.loads(line[7:]).items()})
        print(f"{rows} rows: us per launch group (seed + sweep + fallback + merge), every repeat", flush=True)
        ref = sides[0][0]
        for nb in batches:
            cells = []
            for name, _ in sides:
                v = [r[nb] for r in res[name]]
                cells.append(f"{name} {v}" + ("" if name == ref else f" fastest-{ref} / slowest = {min(r[nb] for r in res[ref]) / max(v):.3f}"))
            print(f"  {nb:3d} batches: " + "  ".join(cells), flush=True)


if __name__ == "__main__":
    main()
