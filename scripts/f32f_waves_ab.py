#!/usr/bin/env python3
"""The bf16 prefilter sweep (scan_f32f_kernel) as one 8-wave workgroup per CU against two 4-wave workgroups per CU, per
launch size: VSEARCH_F32F_WAVES=8 and =4 in alternated processes (the knob is read when the library loads), each timing
search_dev_multi launch groups of 4, 8, 16 and 32 batches of 32 queries (CBW = 1, 2, 4 and 8 column blocks per wave) on
the synthetic SIFT-1M base with HIP events.  Prints every repeat: the figures DESIGN 4.2b chooses NW per CBW from.

    python3 scripts/f32f_waves_ab.py [--repeats 3] [--rows 1000000] [--batches 4,8,16,32]
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="4,8,16,32")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    if args.worker:
        return worker(args.rows, batches)
    res = {8: [], 4: []}
    for rep in range(args.repeats):
        for nw in (8, 4):
            env = dict(os.environ, VSEARCH_F32F_WAVES=str(nw), VSEARCH_SEED_MIN="1")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--rows", str(args.rows), "--batches", args.batches],
                               env=env, check=True, capture_output=True, text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            r = {int(k): v for k, v in json.loads(line[7:]).items()}
            res[nw].append(r)
            print(f"repeat {rep} NW={nw}: " + "  ".join(f"{nb} batches {r[nb]:.2f} us" for nb in batches), flush=True)
    print("us per launch group (seed + sweep + fallback + merge), every repeat; NW = 4 wins where its slowest beats NW = 8's fastest")
    for nb in batches:
        a8, a4 = [r[nb] for r in res[8]], [r[nb] for r in res[4]]
        print(f"{nb:3d} batches (CBW = {max(1, (2 * nb + 7) // 8)}): NW=8 {a8}  NW=4 {a4}  fastest-8 / slowest-4 = {min(a8) / max(a4):.3f}")


if __name__ == "__main__":
    main()
