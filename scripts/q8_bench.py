"""Micro-benchmark of the UFIXED_POINT_8 runner (vs_q8_*): HIP-event time per batch of 32 queries of execute (quantiser +
score matrix, two launches) and of search (+ top-k, k = 5), and the bytes a batch must move, N * dim_b + 32 * N (rows in,
score matrix out; dim_b = dim rounded up to 64), per second of execute as a share of the HBM peak.  One JSON line per
runner; every repeat is listed.  Used under rocprofv3 for the q8 rows of profiles/.

    python scripts/q8_bench.py [--dim 128] [--rows 1000000] [--reps 5]

--dim 128 runs SIFT-shaped rows through vs_q8_create's specialised kernels and, alternating with them in the same process,
through the general kernels (vs_q8_create_nd under VSEARCH_Q8_ND_FORCE=1); any other --dim runs byte-valued random rows
through the general kernels.  The two runners at 128 must return the same score matrix."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

HBM_PEAK_GBS = 8000.0  # as bench.py


def _data(rows, dim, seed):
    rng = np.random.default_rng(seed)
    out = np.empty((rows, dim), dtype=np.float32)
    step = max(1, (1 << 26) // dim)
    for r0 in range(0, rows, step):
        out[r0:r0 + step] = rng.integers(0, 256, size=(min(step, rows - r0), dim), dtype=np.uint8)
    return out


def _forced_general(pkg, base, enc):
    """vs_q8_create_nd with the comparison toggle set: the general runner at dim 128."""
    os.environ["VSEARCH_Q8_ND_FORCE"] = "1"
    try:
        r = pkg.Q8Runner.__new__(pkg.Q8Runner)
        r._h = C.c_void_p()
        e = pkg.Q8Encodings(*enc)
        pkg._check(pkg.lib().vs_q8_create_nd(base.ctypes.data_as(C.c_void_p), base.shape[0], base.shape[1], C.byref(e), 0, 0, C.byref(r._h)))
        return r
    finally:
        del os.environ["VSEARCH_Q8_ND_FORCE"]


def _ev(fn, n):
    for i in range(4):
        fn(i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = ge.load_package()
    N, dim = a.rows, a.dim
    if dim == 128:
        base, q = pkg.synth_sift(N, seed=20251205), pkg.synth_sift(4096, seed=20251206)
    else:
        base, q = _data(N, dim, 1), _data(4096, dim, 2)
    step = max(1, N // 4096)
    enc = (float(q.max()) / 255, float(base.max()) / 255, 0,
           1.05 * float((q[:64].astype(np.float64) @ base[::step].astype(np.float64).T).max()) / 255)
    runners = [("specialised" if dim == 128 else "general", pkg.Q8Runner(base, enc[0], enc[1], 0, enc[3]))]
    if dim == 128:
        runners.append(("general", _forced_general(pkg, base, enc)))
    del base
    qd = torch.from_numpy(q).cuda()
    st = torch.cuda.current_stream().cuda_stream
    npad = (N + 63) // 64 * 64
    sc = torch.empty((32 * npad,), dtype=torch.uint8, device="cuda")
    ids = torch.empty((32 * 32, 5), dtype=torch.int32, device="cuda")
    top = torch.empty((32 * 32, 5), dtype=torch.uint8, device="cuda")
    mats = []
    for _, r in runners:  # the kernels under comparison must agree before they are timed
        r.execute_dev(qd.data_ptr(), 32, sc.data_ptr(), npad, st)
        torch.cuda.synchronize()
        mats.append(sc.clone())
    assert all(torch.equal(m, mats[0]) for m in mats), "specialised and general score matrices differ"
    assert len(torch.unique(mats[0][:N])) > 16, "degenerate encodings"
    del mats
    ex = {name: [] for name, _ in runners}
    se = {name: [] for name, _ in runners}
    for _ in range(a.reps):  # alternating
        for name, r in runners:
            ex[name].append(_ev(lambda i: r.execute_dev(qd.data_ptr() + (i % 128) * 32 * dim * 4, 32, sc.data_ptr(), npad, st), 64))
            se[name].append(_ev(lambda i: r.search_dev(qd.data_ptr(), 32, 32, 5, ids.data_ptr(), top.data_ptr(), st), 4) / 32)
    dim_b = (dim + 63) // 64 * 64
    nbytes = N * dim_b + 32 * N
    for name, r in runners:
        frac = [nbytes / (u * 1e-6) / 1e9 / HBM_PEAK_GBS for u in ex[name]]
        print(json.dumps({"what": "q8_us_per_batch", "kernels": name, "dim": dim, "dim_b": dim_b, "rows": N, "bytes_per_batch": nbytes,
                          "execute_us": [round(u, 2) for u in ex[name]], "hbm_frac": [round(f, 4) for f in frac],
                          "search_us": [round(u, 2) for u in se[name]]}), flush=True)
        r.close()


if __name__ == "__main__":
    main()
