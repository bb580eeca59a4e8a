"""The single-call scan of a general index (scan_one_nd_kernel) at N = 1 M fp32 rows, k = 5, one batch of B = 1
and of B = 16 queries per call, per dimension, three ways in one session:

    one     this library, default route (one scan_one_nd_kernel launch per call)
    off     this library, index created under VSEARCH_ND_ONE=0 (per-batch route: memset, nd_prep_kernel, scan_nd_kernel, merge)
    parent  another checkout's library (--parent-root: a tree of the parent commit with its library built), if given

Per leg and repeat: microseconds per call by HIP events over back-to-back calls, the synchronised single call on the host
clock (median of 20), and the delivered row bytes 4 N dim_p per second as a fraction of the 8 TB/s HBM peak, from the
back-to-back time.  The legs alternate inside every repeat (one, off, parent, one, off, parent, ...): each leg lives in a
worker process of its own that builds its index once and then measures when the driver tells it to, so the three see the
same minutes of the machine.  Before anything is timed the legs' outputs (ids, distance bits, flags) for one call are
compared: a leg that answers differently ends the run.  At dim 128 the general legs run under VSEARCH_ND_FORCE=1 and the
specialised scan_one_kernel (this library, no force) is measured beside them as the yardstick.

    python scripts/nd_one_bench.py [--dims 96,128,384,768,1024,2048] [--rows 1000000] [--reps 5] [--parent-root DIR]

One JSON line per (dimension, B, leg) with every repeat and min / max.

--u8: the single-call BYTE scan (scan_one_nd_i8_kernel) instead: N = 1 M synth_sift rows as uint8 in a from_u8
index, byte-valued synth_sift queries, the same three legs with VSEARCH_ND_ONE_U8=0 as the toggle (per-batch route: reset,
nd_prep_i8_kernel, scan_nd_i8_kernel, merge), and a fourth, `f32`: the default index under precision 1 (the fp32 rows on
scan_one_nd_kernel), for scale.  --dims takes dim[:metric] there (default 96,128:ip,384,384:ip,768,1024,2048; dim 128 is a
general byte index under inner product only).  The check before timing also ends the run if a byte leg refuses a batch
(flags == 2: it would time an empty scan).  Row bytes are N dim_b for the byte legs and 4 N dim_p for `f32`.

    python scripts/nd_one_bench.py --u8 [--parent-root DIR] > profiles/nd_one_u8_bench.txt"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # as bench.py
K = 5


def _data(rows, dim, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=np.float32)
    step = max(1, (1 << 26) // dim)
    for r0 in range(0, rows, step):
        out[r0:r0 + step] = rng.integers(0, 64, size=(min(step, rows - r0), dim), dtype=np.uint8)
    return out


def worker(a):
    """--worker: indexes named in --legs (name or name=ENV=VALUE) over the seeded base; then one command per line on stdin:
    `check B`, `measure NAME B`, `quit`; one JSON line per command on stdout."""
    sys.path.insert(0, a.root)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    base = pkg.synth_sift(a.rows, 1, a.dim).astype(np.uint8) if a.u8 else _data(a.rows, a.dim, 1)
    idx = {}
    for leg in a.legs.split(","):
        name, _, env = leg.partition("=")
        var, _, val = env.partition("=")
        if name == "f32":  # (--u8) the default index once more: measured under precision 1
            idx[name] = idx["one"]
            continue
        if var:
            os.environ[var] = val
        try:
            if a.u8:
                idx[name] = pkg.BruteForceIndex.from_u8(base, metric=a.metric)
                idx[name].set_precision(2)  # (refused if the byte copy was not kept)
            else:
                idx[name] = pkg.BruteForceIndex(base)
                idx[name].set_precision(1)
        finally:
            if var:
                del os.environ[var]
    del base
    qd = torch.from_numpy(pkg.synth_sift(64 * 16, 2, a.dim) if a.u8 else _data(64 * 16, a.dim, 2)).to(dev)
    oi = torch.zeros((16, K + 1), dtype=torch.int32, device=dev)
    od = torch.zeros((16, K + 1), dtype=torch.float32, device=dev)
    fl = torch.zeros((16,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    print(json.dumps({"ready": sorted(idx)}), flush=True)

    def select(name):
        if a.u8:
            idx[name].set_precision(1 if name == "f32" else 2)
        return idx[name]

    def call(ix, B, i):
        ix.search_dev(qd.data_ptr() + (i % 64) * B * a.dim * 4, B, K, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), st)

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "check":  # a digest of the outputs of calls 0..3 of every index, forwards and backwards walks included
            B = int(cmd[1])
            out, refused = {}, []
            for name in idx:
                ix = select(name)
                h = hashlib.sha256()
                for i in range(4):
                    call(ix, B, i)
                    torch.cuda.synchronize()
                    for t in (oi, od, fl):
                        h.update(t[:B].cpu().numpy().tobytes())
                    if (fl[:B] == 2).any().item():
                        refused.append(name)
                out[name] = h.hexdigest()[:16]
            print(json.dumps({"check": out, "refused": refused}), flush=True)
            continue
        name, B = cmd[1], int(cmd[2])
        ix = select(name)
        for i in range(8):
            call(ix, B, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(16):
            call(ix, B, i)
        torch.cuda.synchronize()
        est = (time.perf_counter() - t0) / 16
        n = int(min(2000, max(64, 0.1 / max(est, 1e-6))))  # a window of about 0.1 s
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(ix, B, i)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        lat = []
        for i in range(20):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(ix, B, i)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t)
        print(json.dumps({"us": us, "sync_us": sorted(lat)[len(lat) // 2] * 1e6, "calls": n}), flush=True)
    for ix in idx.values():
        ix.close()


class Worker:
    def __init__(self, a, root, dim, legs, env):
        e = dict(os.environ)
        e.update(env)
        self.legs = [x.partition("=")[0] for x in legs.split(",")]
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--dim", str(dim), "--rows", str(a.rows),
                                   "--legs", legs] + (["--u8", "--metric", str(a.metric)] if a.u8 else []), env=e, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def read(self):
        line = self.p.stdout.readline()
        if not line:  # the worker died: nothing more is started on the GPU
            raise SystemExit(f"worker {self.legs} ended early (exit status {self.p.wait()})")
        return json.loads(line)

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        return self.read()

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="")
    ap.add_argument("--u8", action="store_true", help="the byte scan of a from_u8 index (scan_one_nd_i8_kernel) instead")
    ap.add_argument("--metric", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--dim", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--legs", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.u8:
        return main_u8(a)
    a.dims = a.dims or "96,128,384,768,1024,2048"
    for dim in [int(x) for x in a.dims.split(",")]:
        force = {"VSEARCH_ND_FORCE": "1"} if dim == 128 else {}
        workers = [Worker(a, ROOT, dim, "one,off=VSEARCH_ND_ONE=0", force)]
        if a.parent_root:
            workers.append(Worker(a, os.path.abspath(a.parent_root), dim, "parent", force))
        if dim == 128:
            workers.append(Worker(a, ROOT, dim, "scan_one_kernel", {}))
        try:
            for w in workers:
                w.read()  # ready
            order = [(w, leg) for w in workers for leg in w.legs]
            dim_p = (dim + 15) // 16 * 16
            for B in [int(x) for x in a.batches.split(",")]:
                digests = {}
                for w in workers:
                    digests.update(w.ask(f"check {B}")["check"])
                if len(set(digests.values())) != 1:
                    raise SystemExit(f"dim {dim} B {B}: the legs answer differently: {digests}")
                res = {leg: {"us": [], "sync_us": []} for _, leg in order}
                for _ in range(a.reps):
                    for w, leg in order:
                        m = w.ask(f"measure {leg} {B}")
                        res[leg]["us"].append(m["us"])
                        res[leg]["sync_us"].append(m["sync_us"])
                for _, leg in order:
                    us, sy = res[leg]["us"], res[leg]["sync_us"]
                    row_floats = 128 if leg == "scan_one_kernel" else dim_p
                    print(json.dumps({"dim": dim, "dim_p": dim_p, "rows": a.rows, "B": B, "k": K, "leg": leg,
                                      "us_per_call": [round(x, 2) for x in us], "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                                      "sync_call_us": [round(x, 1) for x in sy], "sync_min": round(min(sy), 1), "sync_max": round(max(sy), 1),
                                      "hbm_frac_best": round(4.0 * a.rows * row_floats / (min(us) * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                      "same_outputs": True}), flush=True)
        finally:
            for w in workers:
                w.close()


def main_u8(a):
    for spec in (a.dims or "96,128:ip,384,384:ip,768,1024,2048").split(","):
        d, _, mname = spec.partition(":")
        dim, a.metric = int(d), 1 if mname == "ip" else 0
        workers = [Worker(a, ROOT, dim, "one,off=VSEARCH_ND_ONE_U8=0,f32", {})]
        if a.parent_root:
            workers.append(Worker(a, os.path.abspath(a.parent_root), dim, "parent", {}))
        try:
            for w in workers:
                w.read()  # ready
            order = [(w, leg) for w in workers for leg in w.legs]
            dim_p, dim_b = (dim + 15) // 16 * 16, (dim + 63) // 64 * 64
            for B in [int(x) for x in a.batches.split(",")]:
                digests = {}
                for w in workers:
                    c = w.ask(f"check {B}")
                    if c["refused"]:
                        raise SystemExit(f"dim {dim} B {B}: a batch was refused (flags == 2) on {c['refused']}")
                    digests.update(c["check"])
                if len(set(digests.values())) != 1:
                    raise SystemExit(f"dim {dim} B {B}: the legs answer differently: {digests}")
                res = {leg: {"us": [], "sync_us": []} for _, leg in order}
                for _ in range(a.reps):
                    for w, leg in order:
                        m = w.ask(f"measure {leg} {B}")
                        res[leg]["us"].append(m["us"])
                        res[leg]["sync_us"].append(m["sync_us"])
                for _, leg in order:
                    us, sy = res[leg]["us"], res[leg]["sync_us"]
                    row_bytes = 4 * dim_p if leg == "f32" else dim_b
                    print(json.dumps({"dim": dim, "dim_b": dim_b, "metric": "ip" if a.metric else "l2", "rows": a.rows, "B": B, "k": K, "leg": leg,
                                      "us_per_call": [round(x, 2) for x in us], "us_min": round(min(us), 2), "us_max": round(max(us), 2),
                                      "sync_call_us": [round(x, 1) for x in sy], "sync_min": round(min(sy), 1), "sync_max": round(max(sy), 1),
                                      "row_bytes": row_bytes,
                                      "hbm_frac_best": round(1.0 * a.rows * row_bytes / (min(us) * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                      "same_outputs": True}), flush=True)
        finally:
            for w in workers:
                w.close()


if __name__ == "__main__":
    main()
