"""bf16 prefilter of a general fp32 index against the same library under VSEARCH_ND_FILTER=0.

N gaussian rows at each dimension, calls of n_batches x 32 queries at k = 10 through search_dev_multi, timed by HIP events;
the two legs run in alternated child processes (the toggle is read at index creation), `--rounds` times each.  Prints per
shape the median and the spread (max - min of the rounds' medians) of both legs, whether ids and distance bits agree, the candidates written and kept per query
and the image's creation time.

    python scripts/nd_filter_bench.py --rows 1000000 --dims 96,128,384,768,1024,2048 --out profiles/nd_filter_bench.txt
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (4, 8, 16, 32)


def child(rows, dim, leg, reps):
    import importlib.util
    import numpy as np
    import torch
    os.environ["VSEARCH_ND_FILTER"] = "2" if leg == "filter" else "0"
    os.environ["VSEARCH_ND_FORCE"] = "1"
    spec = importlib.util.spec_from_file_location("vsearch_pkg", os.path.join(ROOT, "hai-25-rag-on-edge_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    rng = np.random.default_rng(dim)
    base = rng.standard_normal((rows, dim), dtype=np.float32)
    q = torch.from_numpy(rng.standard_normal((32 * 32, dim), dtype=np.float32)).cuda()
    t0 = time.perf_counter()
    idx = pkg.BruteForceIndex(base)
    create_s = time.perf_counter() - t0
    k, res = 10, {"create_s": create_s}
    oi = torch.empty((1024, k + 1), dtype=torch.int32, device="cuda")
    od = torch.empty((1024, k + 1), dtype=torch.float32, device="cuda")
    fl = torch.empty((1024,), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for nb in NBS:
        call = lambda: idx.search_dev_multi(q.data_ptr(), nb, 32, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), s)
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        if leg == "filter":
            idx.filter_stats(reset=True)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        digest = hashlib.sha1(oi[:nb * 32].cpu().numpy().tobytes() + od[:nb * 32].cpu().numpy().tobytes()).hexdigest()
        res[str(nb)] = {"us": statistics.median(ms) * 1e3, "sum": digest}  # ids and distance bits of all k + 1 columns
        if leg == "filter":
            st = idx.filter_stats()
            res[str(nb)].update(overflow=st[1], written=st[2] / (st[0] * nb * 32), kept=st[3] / (st[0] * nb * 32))
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dims", default="96,128,384,768,1024,2048")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--nbs", default="4,8,16,32")
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    global NBS
    NBS = tuple(int(x) for x in a.nbs.split(","))
    if a.child:
        return child(a.rows, int(a.child[0]), a.child[1], int(a.child[2]))
    lines = [f"# rows {a.rows}, k 10, B 32, {a.rounds} alternated rounds x {a.reps} calls; us per call: median (spread)"]
    for dim in [int(d) for d in a.dims.split(",")]:
        runs = {"filter": [], "toggle": []}
        for _ in range(a.rounds):
            for leg in ("filter", "toggle"):
                out = subprocess.run([sys.executable, __file__, "--rows", str(a.rows), "--nbs", a.nbs, "--child", str(dim), leg, str(a.reps)],
                                     capture_output=True, text=True, timeout=900)
                row = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
                if out.returncode != 0 or not row:
                    raise SystemExit(f"child failed (dim {dim}, {leg}, rc {out.returncode}):\n{out.stderr[-2000:]}")
                runs[leg].append(json.loads(row[0][7:]))
        lines.append(f"dim {dim}: image creation + {statistics.median(r['create_s'] for r in runs['filter']) - statistics.median(r['create_s'] for r in runs['toggle']):.2f} s")
        for nb in NBS:
            f = [r[str(nb)]["us"] for r in runs["filter"]]
            t = [r[str(nb)]["us"] for r in runs["toggle"]]
            same = len({r[str(nb)]["sum"] for leg in runs.values() for r in leg}) == 1
            st = runs["filter"][0][str(nb)]
            lines.append(f"  nb {nb:2d}: filter {statistics.median(f):9.1f} ({max(f) - min(f):7.1f})  toggle {statistics.median(t):9.1f} ({max(t) - min(t):7.1f})"
                         f"  x{statistics.median(t) / statistics.median(f):5.2f}  written/q {st['written']:.0f} kept/q {st['kept']:.0f} overflow {st['overflow']}"
                         f"  {'same ids and bits' if same else 'OUTPUTS DIFFER'}")
        print("\n".join(lines[-1 - len(NBS):]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
