"""Micro-benchmark of the UFIXED_POINT_8 runner (vs_q8_*): HIP-event time per batch of 32 queries of execute (quantiser +
score matrix, two launches) and of search (+ top-k, k = 5), and the bytes a batch must move, N * dim_b + 32 * N (rows in,
score matrix out; dim_b = dim rounded up to 64), per second of execute as a share of the HBM peak.  One JSON line per
runner; every repeat is listed.  Used under rocprofv3 for the q8 rows of profiles/.

    python scripts/q8_bench.py [--dim 128] [--rows 1000000] [--reps 5] [--wide-k K [--parent-lib PATH]]

--dim 128 runs SIFT-shaped rows through vs_q8_create's specialised kernels and, alternating with them in the same process,
through the general kernels (vs_q8_create_nd under VSEARCH_Q8_ND_FORCE=1); any other --dim runs byte-valued random rows
through the general kernels.  The two runners at 128 must return the same score matrix.

--wide-k K (17 .. 128) measures the counting select of search_topk_dev instead, on one runner, every leg alternated over the
repeats in one process, HIP-event microseconds per batch of 32 queries:
  (a) search_dev at k = 10 and search_topk_dev at k = K (32 batches per call); with --parent-lib, search_dev at k = 10
      through that other build of libvsearch_hip.so as well (the k <= 16 launches must not have changed)
  (b) the selection alone, topk_scores_dev on the runner's own score matrix: k = 16 (the chunk and final kernels), 17 and K
  (c) the same on an all-255 matrix and on a matrix of two levels at random, the contention cases of the histogram"""
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


def _parent_runner(path, base, enc):
    """A runner of another build of the library, through its C ABI alone: (search_dev(k) closure, close)."""
    L = C.CDLL(path)
    vp = C.c_void_p
    create = L.vs_q8_create if base.shape[1] == 128 else L.vs_q8_create_nd
    create.argtypes = [vp, C.c_int64, C.c_int, vp, C.c_int, C.c_int64, C.POINTER(vp)]
    L.vs_q8_search_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.vs_q8_destroy.argtypes = [vp]
    L.vs_q8_destroy.restype = None
    h = vp()
    e = (C.c_float * 4)()  # vs_q8_encodings: three floats and an int32 of 0 in the third place
    e[0], e[1], e[3] = enc[0], enc[1], enc[3]
    rc = create(base.ctypes.data_as(vp), base.shape[0], base.shape[1], C.cast(e, vp), 0, 0, C.byref(h))
    assert rc == 0, rc

    def search_dev(q_ptr, nb, B, k, ids_ptr, top_ptr, st):
        assert L.vs_q8_search_dev(h, q_ptr, nb, B, k, ids_ptr, top_ptr, st) == 0

    return search_dev, lambda: L.vs_q8_destroy(h)


def wide(a, pkg):
    N, dim, K = a.rows, a.dim, a.wide_k
    if dim == 128:
        base, q = pkg.synth_sift(N, seed=20251205), pkg.synth_sift(4096, seed=20251206)
    else:
        base, q = _data(N, dim, 1), _data(4096, dim, 2)
    step = max(1, N // 4096)
    enc = (float(q.max()) / 255, float(base.max()) / 255, 0,
           1.05 * float((q[:64].astype(np.float64) @ base[::step].astype(np.float64).T).max()) / 255)
    r = pkg.Q8Runner(base, enc[0], enc[1], 0, enc[3])
    parent = _parent_runner(a.parent_lib, base, enc) if a.parent_lib else None
    del base
    qd = torch.from_numpy(q[:1024].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    npad = (N + 63) // 64 * 64
    own = torch.empty((32, npad), dtype=torch.uint8, device="cuda")
    r.execute_dev(qd.data_ptr(), 32, own.data_ptr(), npad, st)
    mats = {"own": own, "all_255": torch.full((32, npad), 255, dtype=torch.uint8, device="cuda"),
            "two_levels": torch.randint(0, 2, (32, npad), dtype=torch.uint8, device="cuda") * 55 + 200}
    ids = torch.empty((1024, 128), dtype=torch.int32, device="cuda")
    top = torch.empty((1024, 128), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert len(torch.unique(own[0, :N])) > 16, "degenerate encodings"
    # what is timed must be right: the wide selection against torch's stable sort on four queries of every matrix
    for name, m in mats.items():
        r.topk_scores_dev(m.data_ptr(), npad, 32, K, ids.data_ptr(), top.data_ptr(), st)
        torch.cuda.synchronize()
        for b in (0, 9, 22, 31):
            v, order = torch.sort(m[b, :N], descending=True, stable=True)
            assert torch.equal(order[:K].int(), ids.view(-1)[b * K:(b + 1) * K]) and torch.equal(v[:K], top.view(-1)[b * K:(b + 1) * K]), name
    legs = {"search_dev_k10": lambda i: r.search_dev(qd.data_ptr(), 32, 32, 10, ids.data_ptr(), top.data_ptr(), st),
            f"search_topk_dev_k{K}": lambda i: r.search_topk_dev(qd.data_ptr(), 32, 32, K, ids.data_ptr(), top.data_ptr(), st)}
    if parent:
        legs["parent_search_dev_k10"] = lambda i: parent[0](qd.data_ptr(), 32, 32, 10, ids.data_ptr(), top.data_ptr(), st)
    per_call = {name: 32 for name in legs}
    for name, m in mats.items():
        for k in (16, 17, K):
            legs[f"select_{name}_k{k}"] = (lambda i, m=m, k=k: r.topk_scores_dev(m.data_ptr(), npad, 32, k, ids.data_ptr(), top.data_ptr(), st))
            per_call[f"select_{name}_k{k}"] = 1
    us = {name: [] for name in legs}
    for _ in range(a.reps):  # alternating
        for name, fn in legs.items():
            us[name].append(_ev(fn, 4 if per_call[name] == 32 else 64) / per_call[name])
    print(json.dumps({"what": "q8_wide_k_us_per_batch", "dim": dim, "rows": N, "B": 32, "wide_k": K, "reps": a.reps,
                      "parent_lib": bool(parent), "us": {n: [round(u, 2) for u in v] for n, v in us.items()}}), flush=True)
    r.close()
    if parent:
        parent[1]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--wide-k", type=int, default=0, help="measure search_topk_dev at this k (17 .. 128) instead")
    ap.add_argument("--parent-lib", default=None, help="with --wide-k: another build of libvsearch_hip.so for the k = 10 leg")
    a = ap.parse_args()
    pkg = ge.load_package()
    if a.wide_k:
        return wide(a, pkg)
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
