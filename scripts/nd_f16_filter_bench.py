"""f16 MFMA prefilter of a float16 index against the same library under VSEARCH_ND_F16_FILTER=0.

N gaussian rows rounded to float16 at each dimension, calls of n_batches x 32 queries at k = 10 through search_dev_multi,
timed by HIP events; the two legs run in alternated child processes (the toggle is read at index creation), `--rounds`
times each.  Prints per shape the median and the spread (max - min of the rounds' medians) of both legs, whether ids and
distance bits agree, and the candidates written and kept per query.  Beside it, claiming nothing, one run of the fp32
index's default route on the widened rows (`--fp32-dims`: the dimensions to run it at).

    python scripts/nd_f16_filter_bench.py --rows 1000000 --dims 96,384,768,1024,2048 --out profiles/nd_f16_filter_bench.txt
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBS = (4, 8, 16, 32)


def half_rows(rows, dim):
    """gaussian rows as float16, drawn in 16 independent streams (the generator, not the GPU, would set the run time)"""
    import numpy as np
    out = np.empty((rows, dim), dtype=np.float16)
    cuts = np.linspace(0, rows, 17).astype(np.int64)
    gens = np.random.default_rng(dim).spawn(16)

    def fill(i):
        for r0 in range(cuts[i], cuts[i + 1], 8192):
            r1 = min(r0 + 8192, cuts[i + 1])
            out[r0:r1] = gens[i].standard_normal((r1 - r0, dim), dtype=np.float32)
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(fill, range(16)))
    return out


def child(rows, dim, leg, reps):
    import importlib.util
    import numpy as np
    import torch
    os.environ["VSEARCH_ND_F16_FILTER"] = "2" if leg == "filter" else "0"
    spec = importlib.util.spec_from_file_location("vsearch_pkg", os.path.join(ROOT, "hai-25-rag-on-edge_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    base = half_rows(rows, dim)
    q = torch.from_numpy(np.random.default_rng(dim + 1).standard_normal((32 * 32, dim), dtype=np.float32)).cuda()
    t0 = time.perf_counter()
    idx = pkg.BruteForceIndex(base.astype(np.float32)) if leg == "fp32" else pkg.BruteForceIndex.from_f16(base)
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
    ap.add_argument("--dims", default="96,384,768,1024,2048")
    ap.add_argument("--fp32-dims", default="96,384,768,1024")
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

    def run(dim, leg):
        out = subprocess.run([sys.executable, __file__, "--rows", str(a.rows), "--nbs", a.nbs, "--child", str(dim), leg, str(a.reps)],
                             capture_output=True, text=True, timeout=300)
        row = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not row:
            raise SystemExit(f"child failed (dim {dim}, {leg}, rc {out.returncode}):\n{out.stderr[-2000:]}")
        return json.loads(row[0][7:])

    fp32_dims = [int(d) for d in a.fp32_dims.split(",") if d]
    lines = [f"# rows {a.rows}, float16, k 10, B 32, {a.rounds} alternated rounds x {a.reps} calls; us per call: median (spread)"]
    for dim in [int(d) for d in a.dims.split(",")]:
        runs = {"filter": [], "toggle": []}
        for _ in range(a.rounds):
            for leg in ("filter", "toggle"):
                runs[leg].append(run(dim, leg))
        fp32 = run(dim, "fp32") if dim in fp32_dims else None
        n0 = len(lines)
        lines.append(f"dim {dim}: creation + {statistics.median(r['create_s'] for r in runs['filter']) - statistics.median(r['create_s'] for r in runs['toggle']):.2f} s")
        for nb in NBS:
            f = [r[str(nb)]["us"] for r in runs["filter"]]
            t = [r[str(nb)]["us"] for r in runs["toggle"]]
            same = len({r[str(nb)]["sum"] for leg in runs.values() for r in leg}) == 1
            st = runs["filter"][0][str(nb)]
            lines.append(f"  nb {nb:2d}: filter {statistics.median(f):9.1f} ({max(f) - min(f):7.1f})  toggle {statistics.median(t):9.1f} ({max(t) - min(t):7.1f})"
                         f"  x{statistics.median(t) / statistics.median(f):5.2f}  written/q {st['written']:.0f} kept/q {st['kept']:.0f} overflow {st['overflow']}"
                         f"  {'same ids and bits' if same else 'OUTPUTS DIFFER'}"
                         + (f"  | fp32 index, default route, one run: {fp32[str(nb)]['us']:9.1f}"
                            f"{'' if fp32[str(nb)]['sum'] == runs['toggle'][0][str(nb)]['sum'] else ' (OUTPUTS DIFFER)'}" if fp32 else ""))
        print("\n".join(lines[n0:]), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
