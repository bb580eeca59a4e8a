"""The two-launch route of short IVF calls (ivf_one_coarse_kernel + ivf_one_scan_kernel) at N = 1 M fp32 rows
(synth_sift rows as in scripts/ivf_nd_bench.py; --data mixture: tight Gaussians, IVF's best case), index from the library's
builder at nlist 1024, k = 10, one batch of B = 1 and of B = 16 queries per call, nprobe 8, 32, 128 and 256 (the whole range
of the rule), per dimension, against everything it has to be compared with, in one session:

    one     this library, default route (two launches per call)
    off     this library, index created under VSEARCH_IVF_ONE=0 (the group route: ten launches per call)
    parent  another checkout's library (--parent-root: a tree of the parent commit with its library built), if given
    exact   scan_one_nd_kernel on the same rows (BruteForceIndex, fp32): exact search, the figure IVF has to beat
    spec128 at dim 128 only: the specialised 128-d IVF index (the general legs run under VSEARCH_IVF_ND_FORCE=1 there)

Per leg and repeat: microseconds per call by HIP events over back-to-back calls and the synchronised single call on the
host clock (median of 20).  Every leg lives in a worker process of its own that builds its index once (the same seeded
rows, the same builder call: the same index) and then measures when the driver tells it to; the legs alternate inside every
repeat, so they see the same minutes of the machine.  Before anything is timed the IVF legs' outputs for four calls are
compared (ids and distance bits): a leg that answers differently ends the run.  recall@10 of the IVF answer against the
exact one is reported per nprobe over 256 queries.

    python scripts/ivf_one_bench.py [--dims 96,128,384,768] [--rows 1000000] [--nlist 1024] [--reps 5] [--parent-root DIR]
                                    [--out profiles/ivf_one_bench.txt]
    python scripts/ivf_one_bench.py --u8 [--u8-unit-root DIR] [--batches 1,8,16] [--out profiles/ivf_one_u8_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python scripts/ivf_one_bench.py --one DIM,B,NPROBE

--u8: the byte route (ivf_one_coarse_kernel in its byte-index mode + ivf_one_scan_u8_kernel) on the same index
built from the same rows as uint8 (IVFIndex.from_u8; synth_sift rows are byte valued), against its two alternatives:

    u8      the byte route at every shape of vs_ivf_one_plan's rule (VSEARCH_IVF_ONE_U8=2: the shapes vs_ivf_one_plan_u8 takes
            out included -- the column `rule` says what vs_ivf_one_plan_u8 makes of the shape)
    u8f32   the SAME index in the same process under set_precision(1): the fp32 two-launch route
    u8off   the same index created under VSEARCH_IVF_ONE_U8=0 in a process of its own: the group route on the byte rows
    u8unit  with --u8-unit-root DIR: the same leg on another build of this tree (EXTRA=-DVS_IVF_ONE_U8_UNIT_ROWS=2048: byte
            units of 2048 rows), a process of its own
    parent  with --parent-root: the parent commit's library on the same index (its group route on the byte rows)

and, for B = 1, the probed rows' bytes over the WHOLE call's time: total_candidates x dim_b bytes (dim_p x 4 for u8f32).  (With
more queries total_candidates counts a list once per query that probes it, not once per read: no such figure is printed.)

One JSON line per (dimension, nprobe, B, leg) with every repeat, min and median; --out writes the same as a table.  --one
runs 320 calls of one shape in one process: the run to profile for the per-launch split (coarse, scan)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10
NQ = 1024  # queries on the device: calls walk through them


def _data(rows, dim, nlist, seed, kind="sift", pkg=None):
    """sift: synth_sift rows, the data of scripts/ivf_nd_bench.py (recall@10 well under 1 at nprobe 8).  mixture: nlist tight
    Gaussians (sigma 0.35 around N(0, 1) centres), the best case for IVF and for the scan's bound: recall 1.0"""
    if kind == "sift":
        return pkg.synth_sift(rows, seed=seed, dim=dim)
    rng = np.random.default_rng(seed)
    centres = np.random.default_rng(7).standard_normal((nlist, dim)).astype(np.float32)
    out = np.empty((rows, dim), dtype=np.float32)
    step = max(1, (1 << 25) // dim)
    for r0 in range(0, rows, step):
        n = min(step, rows - r0)
        out[r0:r0 + n] = centres[rng.integers(0, nlist, size=n)] + 0.35 * rng.standard_normal((n, dim), dtype=np.float32)
    return out


def worker(a):
    """--worker: one index over the seeded base (--kind ivf | bf); then one command per line on stdin: `check B nprobe`,
    `measure B nprobe`, `answers nprobe`, `quit`; one JSON line per command on stdout."""
    sys.path.insert(0, a.root)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    base = _data(a.rows, a.dim, a.nlist, 1, a.data, pkg)
    if a.kind == "bf":
        ix = pkg.BruteForceIndex(base)
        ix.set_precision(1)
        kk = K + 1
    elif a.kind == "ivfu8":
        vr, off, r2o, cents, _ = pkg.ivf_build(base, a.nlist, 4, 1e-4, 42, 0)
        u8 = vr.astype(np.uint8)
        assert np.array_equal(u8.astype(np.float32), vr), "--u8 needs byte-valued rows"
        ix = pkg.IVFIndex.from_u8(u8, cents, off, r2o)
        kk = K
        del vr, u8
    else:
        vr, off, r2o, cents, _ = pkg.ivf_build(base, a.nlist, 4, 1e-4, 42, 0)
        ix = pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o)
        ix.set_precision(1)
        kk = K
        del vr
    del base
    qd = torch.from_numpy(_data(NQ, a.dim, a.nlist, 2, a.data, pkg)).to(dev)
    oi = torch.zeros((NQ, kk), dtype=torch.int32, device=dev)
    od = torch.zeros((NQ, kk), dtype=torch.float32, device=dev)
    fl = torch.zeros((NQ,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    print(json.dumps({"ready": a.kind}), flush=True)

    def call(B, nprobe, i, o=0):
        q = qd.data_ptr() + (i % (NQ // B)) * B * a.dim * 4
        if a.kind == "bf":
            ix.search_dev(q, B, K, oi.data_ptr() + o * kk * 4, od.data_ptr() + o * kk * 4, fl.data_ptr(), st)
        else:
            ix.search_dev(q, B, K, nprobe, oi.data_ptr() + o * kk * 4, od.data_ptr() + o * kk * 4, st)

    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "check":  # a digest of the outputs of calls 0..3
            B, nprobe = int(cmd[1]), int(cmd[2])
            h = hashlib.sha256()
            for i in range(4):
                call(B, nprobe, i)
                torch.cuda.synchronize()
                for t in (oi, od):
                    h.update(t[:B].cpu().numpy().tobytes())
            print(json.dumps({"check": h.hexdigest()[:16]}), flush=True)
            continue
        if cmd[0] == "precision":  # (--u8: the same index on the fp32 two-launch route and back)
            ix.set_precision(int(cmd[1]))
            print(json.dumps({"precision": int(cmd[1])}), flush=True)
            continue
        if cmd[0] == "route":  # (--u8) what the counters say the last calls took, cleared; candidate rows of one call of the shape
            B, nprobe = int(cmd[1]), int(cmd[2])
            one = list(ix.one_stats(reset=True))
            one8 = list(ix.one_u8_stats(reset=True)) if hasattr(ix, "one_u8_stats") else None
            nd = list(ix.nd_u8_stats(reset=True))
            rows = ix.searchBatch(qd[:B].cpu().numpy(), B, K, nprobe)[2]
            ix.one_stats(reset=True)  # (that call is not one of the measured ones)
            if one8 is not None:
                ix.one_u8_stats(reset=True)
            ix.nd_u8_stats(reset=True)
            print(json.dumps({"one": one, "one_u8": one8, "nd_u8": nd, "rows": int(rows)}), flush=True)
            continue
        if cmd[0] == "answers":  # the ids of the first 256 queries, one query per call
            nprobe = int(cmd[1])
            for i in range(256):
                call(1, nprobe, i, i)
            torch.cuda.synchronize()
            print(json.dumps({"ids": oi[:256, :K].cpu().numpy().tolist(), "stats": list(ix.one_stats()) if a.kind == "ivf" and hasattr(ix, "one_stats") and a.dim_general else None}), flush=True)
            continue
        B, nprobe = int(cmd[1]), int(cmd[2])
        for i in range(8):
            call(B, nprobe, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(16):
            call(B, nprobe, i)
        torch.cuda.synchronize()
        est = (time.perf_counter() - t0) / 16
        n = int(min(2000, max(64, 0.1 / max(est, 1e-6))))  # a window of about 0.1 s
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            call(B, nprobe, i)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        lat = []
        for i in range(20):
            torch.cuda.synchronize()
            t = time.perf_counter()
            call(B, nprobe, i)
            torch.cuda.synchronize()
            lat.append(time.perf_counter() - t)
        print(json.dumps({"us": us, "sync_us": sorted(lat)[len(lat) // 2] * 1e6, "calls": n}), flush=True)
    ix.close()


def one_shape(a):
    """--one DIM,B,NPROBE: build the index, 20 warm-up calls and 300 timed ones of that shape, nothing else on the device"""
    sys.path.insert(0, a.root)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dim, B, nprobe = [int(x) for x in a.one.split(",")]
    base = _data(a.rows, dim, a.nlist, 1, a.data, pkg)
    vr, off, r2o, cents, _ = pkg.ivf_build(base, a.nlist, 4, 1e-4, 42, 0)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(_data(NQ, dim, a.nlist, 2, a.data, pkg)).to(dev)
    oi = torch.zeros((B, K), dtype=torch.int32, device=dev)
    od = torch.zeros((B, K), dtype=torch.float32, device=dev)
    with pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o) as ix:
        for i in range(320):
            ix.search_dev(qd.data_ptr() + (i % (NQ // B)) * B * dim * 4, B, K, nprobe, oi.data_ptr(), od.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        print(json.dumps({"one": a.one, "one_stats": list(ix.one_stats())}))


class Worker:
    def __init__(self, a, name, root, dim, kind, env, general):
        e = dict(os.environ)
        for v in ("VSEARCH_IVF_ONE", "VSEARCH_IVF_ONE_U8", "VSEARCH_IVF_ND_FORCE"):
            e.pop(v, None)
        e.update(env)
        self.name, self.kind = name, kind
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--dim", str(dim), "--rows", str(a.rows),
                                   "--nlist", str(a.nlist), "--kind", kind, "--data", a.data] + (["--dim-general"] if general else []),
                                  env=e, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def read(self):
        line = self.p.stdout.readline()
        if not line:  # the worker died: nothing more is started on the GPU
            raise SystemExit(f"worker {self.name} ended early (exit status {self.p.wait()})")
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


def main_u8(a):
    """--u8: see the module's text"""
    table = [f"# python3 scripts/ivf_one_bench.py --u8 --dims {a.dims} --rows {a.rows} --nlist {a.nlist} --reps {a.reps} --nprobes {a.nprobes} --data {a.data}"
             + (" --u8-unit-root <this tree built with EXTRA=-DVS_IVF_ONE_U8_UNIT_ROWS=2048>" if a.u8_unit_root else "") + (" --parent-root <a checkout of the parent commit, library built>" if a.parent_root else ""),
             "# us per call back to back by HIP events (min, median over the alternations) | synchronised single call, host clock (median) |",
             "# GB/s (B = 1 only) = probed rows x bytes per padded row of the kind the leg reads / us min, the whole call | route: batches the",
             "# counters saw (byte route, fp32 route) | rule: vs_ivf_one_plan_u8's route for the shape (2 = the byte route, 0 = the group route)",
             f"{'dim':>4} {'nprobe':>6} {'B':>3} {'leg':>7} {'us min':>8} {'us med':>8} {'sync med':>9} {'GB/s':>7} {'route':>9} {'rule':>4}  us per repeat"]
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    plan_u8 = ge.load_package().ivf_one_plan_u8
    for dim in [int(x) for x in a.dims.split(",")]:
        force = {"VSEARCH_IVF_ND_FORCE": "1"} if dim == 128 else {}
        workers = [Worker(a, "u8", ROOT, dim, "ivfu8", dict(force, VSEARCH_IVF_ONE_U8="2"), True),
                   Worker(a, "u8off", ROOT, dim, "ivfu8", dict(force, VSEARCH_IVF_ONE_U8="0"), True)]
        if a.u8_unit_root:
            workers.append(Worker(a, "u8unit", os.path.abspath(a.u8_unit_root), dim, "ivfu8", dict(force, VSEARCH_IVF_ONE_U8="2"), True))
        if a.parent_root:
            workers.append(Worker(a, "parent", os.path.abspath(a.parent_root), dim, "ivfu8", force, False))
        legs = [(w.name, w, None) for w in workers]
        legs.insert(1, ("u8f32", workers[0], 1))
        dim_b, dim_p = (dim + 63) // 64 * 64, (dim + 15) // 16 * 16
        try:
            for w in workers:
                w.read()  # ready
            for nprobe in [int(x) for x in a.nprobes.split(",")]:
                for B in [int(x) for x in a.batches.split(",")]:
                    digests = {}
                    for name, w, prec in legs:
                        if prec is not None:
                            w.ask(f"precision {prec}")
                        digests[name] = w.ask(f"check {B} {nprobe}")["check"]
                        if prec is not None:
                            w.ask("precision 0")
                    if len(set(digests.values())) != 1:
                        raise SystemExit(f"dim {dim} nprobe {nprobe} B {B}: the legs answer differently: {digests}")
                    res = {name: {"us": [], "sync_us": []} for name, _, _ in legs}
                    route = {}
                    for w in workers:
                        if w.name != "parent":
                            w.ask(f"route {B} {nprobe}")  # (clears the counters)
                    for _ in range(a.reps):
                        for name, w, prec in legs:
                            if prec is not None:
                                w.ask(f"precision {prec}")
                            m = w.ask(f"measure {B} {nprobe}")
                            res[name]["us"].append(m["us"])
                            res[name]["sync_us"].append(m["sync_us"])
                            if name != "parent":
                                route[name] = w.ask(f"route {B} {nprobe}")
                            if prec is not None:
                                w.ask("precision 0")
                    for name, w, prec in legs:
                        us, sy = res[name]["us"], res[name]["sync_us"]
                        r = route.get(name)
                        rows = route["u8"]["rows"]
                        gbs = rows * (4 * dim_p if name == "u8f32" else dim_b) / min(us) / 1e3 if B == 1 else 0.0
                        rule = plan_u8(a.rows, dim, a.nlist, 256, 1, B, K, nprobe)[0]
                        rt = f"{r['one_u8'][0] if r['one_u8'] else 0},{r['one'][0]}" if r else "-"
                        print(json.dumps({"dim": dim, "rows": a.rows, "nlist": a.nlist, "nprobe": nprobe, "B": B, "k": K, "leg": name,
                                          "us_per_call": [round(x, 2) for x in us], "us_min": round(min(us), 2), "us_median": round(statistics.median(us), 2),
                                          "sync_median": round(statistics.median(sy), 1), "probed_rows": rows, "gb_per_s": round(gbs, 1), "route": r, "rule": rule,
                                          "same_outputs": True}), flush=True)
                        table.append(f"{dim:>4} {nprobe:>6} {B:>3} {name:>7} {min(us):>8.2f} {statistics.median(us):>8.2f} {statistics.median(sy):>9.1f} "
                                     f"{(f'{gbs:.1f}' if B == 1 else '-'):>7} {rt:>9} {rule:>4}  {[round(x, 1) for x in us]}")
                        if a.out:
                            with open(a.out, "w") as f:
                                f.write("\n".join(table) + "\n")
        finally:
            for w in workers:
                w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="96,128,384,768")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--nprobes", default="8,32,128,256")
    ap.add_argument("--data", default="sift", choices=["sift", "mixture"])
    ap.add_argument("--out", default="", help="also write the table (profiles/ivf_one_bench.txt's form) to this file")
    ap.add_argument("--one", default="", metavar="DIM,B,NPROBE", help="one process, 300 calls of one shape on the default route: "
                    "the run to put under rocprofv3 --kernel-trace --stats for the per-launch split")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built")
    ap.add_argument("--u8", action="store_true", help="the byte route's leg: the index from the same rows as uint8 (DESIGN 4.6e)")
    ap.add_argument("--u8-unit-root", default="", metavar="DIR", help="--u8: one more leg on this tree built with another byte unit size")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--dim", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--kind", default="ivf", help=argparse.SUPPRESS)
    ap.add_argument("--dim-general", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if a.one:
        return one_shape(a)
    if a.u8:
        return main_u8(a)
    table = [f"# python3 scripts/ivf_one_bench.py --dims {a.dims} --rows {a.rows} --nlist {a.nlist} --reps {a.reps} --nprobes {a.nprobes} --data {a.data}"
             + (" --parent-root <a checkout of the parent commit, library built>" if a.parent_root else ""),
             "# us per call back to back by HIP events (min, median over the alternations) | synchronised single call, host clock (median)",
             f"{'dim':>4} {'nprobe':>6} {'B':>3} {'leg':>8} {'us min':>8} {'us med':>8} {'sync med':>9} {'recall@10':>9}  us per repeat"]
    for dim in [int(x) for x in a.dims.split(",")]:
        force = {"VSEARCH_IVF_ND_FORCE": "1"} if dim == 128 else {}
        workers = [Worker(a, "one", ROOT, dim, "ivf", force, True), Worker(a, "off", ROOT, dim, "ivf", dict(force, VSEARCH_IVF_ONE="0"), True)]
        if a.parent_root:
            workers.append(Worker(a, "parent", os.path.abspath(a.parent_root), dim, "ivf", force, False))
        workers.append(Worker(a, "exact", ROOT, dim, "bf", {}, False))
        if dim == 128:
            workers.append(Worker(a, "spec128", ROOT, dim, "ivf", {}, False))
        try:
            for w in workers:
                w.read()  # ready
            ivf = [w for w in workers if w.kind == "ivf"]
            exact = next(w for w in workers if w.name == "exact")
            truth = np.array(exact.ask("answers 0")["ids"])
            for nprobe in [int(x) for x in a.nprobes.split(",")]:
                ans = workers[0].ask(f"answers {nprobe}")
                got = np.array(ans["ids"])
                recall = float(np.mean([len(set(got[i]) & set(truth[i])) / K for i in range(len(truth))]))
                for B in [int(x) for x in a.batches.split(",")]:
                    digests = {w.name: w.ask(f"check {B} {nprobe}")["check"] for w in ivf}
                    if len(set(digests.values())) != 1:
                        raise SystemExit(f"dim {dim} nprobe {nprobe} B {B}: the legs answer differently: {digests}")
                    res = {w.name: {"us": [], "sync_us": []} for w in workers}
                    for _ in range(a.reps):
                        for w in workers:
                            m = w.ask(f"measure {B} {nprobe}")
                            res[w.name]["us"].append(m["us"])
                            res[w.name]["sync_us"].append(m["sync_us"])
                    for w in workers:
                        us, sy = res[w.name]["us"], res[w.name]["sync_us"]
                        print(json.dumps({"dim": dim, "rows": a.rows, "nlist": a.nlist, "nprobe": nprobe if w.kind == "ivf" else None, "B": B, "k": K,
                                          "leg": w.name, "us_per_call": [round(x, 2) for x in us], "us_min": round(min(us), 2),
                                          "us_median": round(statistics.median(us), 2), "sync_call_us": [round(x, 1) for x in sy],
                                          "sync_min": round(min(sy), 1), "sync_median": round(statistics.median(sy), 1),
                                          "recall_at_10": round(recall, 4) if w.kind == "ivf" else 1.0,
                                          "one_stats": ans["stats"] if w.name == "one" else None, "same_outputs": True}), flush=True)
                        table.append(f"{dim:>4} {str(nprobe) if w.kind == 'ivf' else '-':>6} {B:>3} {w.name:>8} {min(us):>8.2f} {statistics.median(us):>8.2f} "
                                     f"{statistics.median(sy):>9.1f} {(recall if w.kind == 'ivf' else 1.0):>9.4f}  {[round(x, 1) for x in us]}")
                        if a.out:
                            with open(a.out, "w") as f:
                                f.write("\n".join(table) + "\n")
        finally:
            for w in workers:
                w.close()


if __name__ == "__main__":
    main()
