"""Exact brute-force search at any vector length 1 <= dim <= 2048 (vs_bf_create_nd, scan_nd_kernel) against the CPU oracle.

Integer-valued data keeps the bit-for-bit claim at any dimension as long as the three quantities of the epilogue
(||q||^2, ||b||^2, q.b) are exact in fp32: values in [0, hi) with 2 dim (hi - 1)^2 < 2^24, hi capped at 256.  Uniform rows
almost never tie above dim 3, so every exactness test plants duplicates (5 % of the rows, at both ends of the base) and
queries that are duplicated rows: the tie resolver runs (timing.tie_queries > 0)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 20, 96, 100, 130, 256, 384, 768, 960, 1024, 1536, 2048]


def _hi(dim):
    hi = min(int(math.isqrt((2 ** 23 - 1) // dim)) + 1, 256)
    assert 2 * dim * (hi - 1) ** 2 < 2 ** 24
    return hi


def test_value_ranges():
    """hi = 256 up to dim 129, then 182 / 148 / 105 / 94 / 91 / 74 / 64 at dim 256 / 384 / 768 / 960 / 1024 / 1536 / 2048."""
    assert [_hi(d) for d in (129, 256, 384, 768, 960, 1024, 1536, 2048)] == [256, 182, 148, 105, 94, 91, 74, 64]


def _int_data(rng, n, nq, dim, hi=None, dup=0.05):
    hi = hi or _hi(dim)
    base = rng.integers(0, hi, size=(n, dim)).astype(np.float32)
    q = rng.integers(0, hi, size=(nq, dim)).astype(np.float32)
    m = int(n * dup / 2)
    if m > 0 and n >= 8 * m:
        # duplicates at both ends of the base, copied from rows of the middle
        src = rng.integers(2 * m, n - 2 * m, size=2 * m)
        base[:m] = base[src[:m]]
        base[n - m:] = base[src[m:]]
        for j in range(min(4, nq)):  # queries that ARE duplicated rows: their two best are tied at 0
            q[j] = base[src[j]]
    return base, q


def _check_exact(pkg, base, q, ks, batch=None, want_ties=True):
    with pkg.BruteForceIndex(base) as idx:
        assert idx.getDim() == base.shape[1] and idx.getNumDocs() == base.shape[0]
        if batch:
            idx.set_batch(batch)
        for k in ks:
            oi, od = oracle.search_bf(base, q, k)
            tm = pkg.Timing()
            ids, d = idx.search(q, k, tm)
            tag = f"(N={base.shape[0]}, dim={base.shape[1]}, nq={len(q)}, k={k}, batch={batch})"
            assert np.array_equal(d, od), "dists differ " + tag
            assert np.array_equal(ids, oi), "ids differ " + tag
            if want_ties:
                assert tm.tie_queries > 0, "the tie resolver did not run " + tag


@pytest.mark.parametrize("dim", DIMS)
def test_exact_at_every_dimension(gpu_pkg, dim):
    rng = np.random.default_rng(1000 + dim)
    base, q = _int_data(rng, 20000, 70, dim)
    _check_exact(gpu_pkg, base, q, (1, 5, 15))


@pytest.mark.parametrize("dim", [100, 960])
@pytest.mark.parametrize("n", [1, 5, 17, 4099])
def test_ragged_bases(gpu_pkg, dim, n):
    rng = np.random.default_rng(2000 + dim + n)
    base, q = _int_data(rng, n, 33, dim)
    if n >= 2:
        base[n - 1] = base[0]
        q[0] = base[0]
    _check_exact(gpu_pkg, base, q, (min(5, n),), want_ties=n >= 2)


@pytest.mark.parametrize("batch", [1, 7, 16, 17, 32])
def test_batch_sizes_at_dim_384(gpu_pkg, batch):
    rng = np.random.default_rng(3000 + batch)
    base, q = _int_data(rng, 20000, 70, 384)
    _check_exact(gpu_pkg, base, q, (5,), batch=batch)


@pytest.mark.parametrize("dim", [96, 960])
@pytest.mark.parametrize("k", [16, 50, 128])
def test_wide_k(gpu_pkg, dim, k):
    """search_topk against oracle.search_bf: slot order among equal distances, stably sorted (as tests/test_gpu_topk_wide.py)."""
    rng = np.random.default_rng(4000 + dim + k)
    base, q = _int_data(rng, 30000, 40, dim)
    oi, od = oracle.search_bf(base, q, k)
    with gpu_pkg.BruteForceIndex(base) as idx:
        tm = gpu_pkg.Timing()
        ids, d = idx.search_topk(q, k, tm)
    assert np.array_equal(d, od)
    assert np.array_equal(ids, oi)
    assert tm.tie_queries > 0


def test_wide_k_candidate_overflow(gpu_pkg):
    """A run of several hundred equal rows next to a query: the filtered pass overflows its candidate list (or the tie
    resolver's) and the dense fallback gives the answer."""
    rng = np.random.default_rng(4500)
    dim = 960
    base, q = _int_data(rng, 30000, 40, dim)
    base[9000:9000 + 700] = base[123]
    base[20000:20000 + 9000] = base[456]  # more equal rows than any candidate list holds
    q[5] = base[123]
    q[6] = base[456]
    for k in (50, 128):
        oi, od = oracle.search_bf(base, q, k)
        with gpu_pkg.BruteForceIndex(base) as idx:
            ids, d = idx.search_topk(q, k)
        assert np.array_equal(d, od), k
        assert np.array_equal(ids, oi), k


def test_search_dev_multi_at_dim_768(gpu_pkg):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5000)
    dim, nb, B, k = 768, 9, 32, 5
    base, q = _int_data(rng, 20000, nb * B, dim)
    s = torch.cuda.current_stream().cuda_stream
    qd = torch.from_numpy(q).to(dev)
    ids = torch.full((nb * B, k + 1), -7, dtype=torch.int32, device=dev)
    d = torch.zeros((nb * B, k + 1), dtype=torch.float32, device=dev)
    fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.search_dev_multi(qd.data_ptr(), nb, B, k, ids.data_ptr(), d.data_ptr(), fl.data_ptr(), s)
        torch.cuda.synchronize()
    oi, od = oracle.search_bf(base, q, k + 1)
    assert np.array_equal(d.cpu().numpy(), od)
    flags = fl.cpu().numpy()
    assert np.array_equal(flags != 0, (od[:, 1:] == od[:, :-1]).any(1))
    assert (flags == 0).sum() > 0 and (flags != 0).sum() > 0
    assert np.array_equal(ids.cpu().numpy()[flags == 0], oi[flags == 0])


def test_scores_dev_at_dim_100(gpu_pkg):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5100)
    n, B, ld = 12345, 20, 12352
    base, q = _int_data(rng, n, B, 100)
    s = torch.cuda.current_stream().cuda_stream
    sc = torch.full((B, ld), -1.0, dtype=torch.float32, device=dev)
    qd = torch.from_numpy(q).to(dev)
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.scores_dev(qd.data_ptr(), B, sc.data_ptr(), ld, s)
        torch.cuda.synchronize()
    got = sc.cpu().numpy()
    want = np.stack([oracle.l2_row(q[i], base) for i in range(B)])
    assert np.array_equal(got[:, :n], want)
    assert np.all(got[:, n:] == -1.0)  # padding columns untouched


@pytest.mark.parametrize("dim", [1, 3, 20, 100, 128, 130, 384, 2048])
def test_score_matrix_is_the_chain_oracles_bits(gpu_pkg, dim):
    """The direct evidence for the arithmetic contract of every fp32 MFMA kernel: on N(0, 1) rows the score matrix equals,
    bit for bit, the oracle's "chain" order -- q.b as one fmaf chain over the elements 16 c + 4 g + i (c ascending, i =
    0..3, g = 0..3 the MFMA's k index), norms in the 8-lane order, fmaf(-2, q.b, |q|^2 + |b|^2) -- and does not equal the
    "lanes8" order.  300 rows = four full 64-row blocks and a ragged one; 100-d is 7 segments (the single-segment tail),
    128-d the specialised index (scan_kernel's store mode, also the coarse stage of an IVF index above 4096 lists)."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8000 + dim)
    n, B, ld = 300, 20, 320
    base = rng.normal(0, 1, size=(n, dim)).astype(np.float32)
    q = rng.normal(0, 1, size=(B, dim)).astype(np.float32)
    want = oracle.l2_matrix(q, base, "chain")
    other = oracle.l2_matrix(q, base, "lanes8")
    if dim >= 20:  # (one or three products: every order is the same chain)
        assert not np.array_equal(want.view(np.int32), other.view(np.int32))
    sc = torch.full((B, ld), -1.0, dtype=torch.float32, device=dev)
    qd = torch.from_numpy(q).to(dev)
    with gpu_pkg.BruteForceIndex(base) as idx:
        assert idx.getDim() == dim
        idx.scores_dev(qd.data_ptr(), B, sc.data_ptr(), ld, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = sc.cpu().numpy()[:, :n].copy()
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    print(f"dim {dim}: {len(bad)} of {got.size} scores differ from the chain order, "
          f"{int((got.view(np.int32) != other.view(np.int32)).sum())} from lanes8")
    if len(bad):
        i, j = bad[0]
        print(f"first: query {i} row {j}: device {float(got[i, j])!r} ({got.view(np.int32)[i, j]:#x}) "
              f"chain {float(want[i, j])!r} ({want.view(np.int32)[i, j]:#x}) lanes8 {float(other[i, j])!r}")
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if dim >= 20:
        assert not np.array_equal(got.view(np.int32), other.view(np.int32))


def test_search_topk_dev_multi_k100(gpu_pkg):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5200)
    dim, nb, B, k = 384, 3, 32, 100
    base, q = _int_data(rng, 30000, nb * B, dim)
    s = torch.cuda.current_stream().cuda_stream
    qd = torch.from_numpy(q).to(dev)
    ids = torch.full((nb * B, k + 1), -7, dtype=torch.int32, device=dev)
    d = torch.zeros((nb * B, k + 1), dtype=torch.float32, device=dev)
    fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.search_topk_dev_multi(qd.data_ptr(), nb, B, k, ids.data_ptr(), d.data_ptr(), fl.data_ptr(), s)
        torch.cuda.synchronize()
    oi, od = oracle.search_bf(base, q, k + 1)
    assert np.array_equal(d.cpu().numpy(), od)
    flags = fl.cpu().numpy()
    assert np.array_equal(flags != 0, (od[:, 1:] == od[:, :-1]).any(1))
    assert np.array_equal(ids.cpu().numpy()[flags == 0], oi[flags == 0])


def test_inner_product_at_dim_384(gpu_pkg):
    rng = np.random.default_rng(6000)
    dim, hi = 384, 100
    base = rng.integers(0, hi, size=(3000, dim)).astype(np.float32)
    q = rng.integers(0, hi, size=(10, dim)).astype(np.float32)
    base[:, 0] += np.arange(3000) % 7  # break ties
    assert dim * (hi - 1 + 6) ** 2 < 2 ** 24
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP) as idx:
        ids, s = idx.search(q, 5)
    ip = q.astype(np.int64) @ base.astype(np.int64).T
    order = np.argsort(-ip, axis=1, kind="stable")[:, :5]
    assert np.array_equal(np.take_along_axis(ip, ids.astype(np.int64), 1), np.take_along_axis(ip, order, 1))
    assert np.array_equal(s, np.take_along_axis(ip, order, 1).astype(np.float32))


def _gaussian_with_planted_neighbours(rng, n, nq, dim):
    """N(0, 1) rows and queries; every query also gets seven rows at squared distances j * 0.04 * dim (j = 1..7) in
    random directions.  Plain N(0, 1) rows alone leave the oracle's own top-5 gaps under 4 x the derived tolerance for
    more than 10 % of the (query, rank) pairs at dim 768 (81 % pass at 20 000 rows, 89 % at 2 000), so the data carries
    its well-separated neighbours with it; the tolerance and the 90 % cap are untouched."""
    base = rng.normal(0, 1, size=(n, dim)).astype(np.float32)
    q = rng.normal(0, 1, size=(nq, dim)).astype(np.float32)
    pos = rng.choice(n, size=nq * 7, replace=False)
    for i in range(nq):
        for j in range(7):
            u = rng.normal(0, 1, size=dim)
            u /= np.linalg.norm(u)
            base[pos[i * 7 + j]] = (q[i] + math.sqrt(0.04 * dim * (j + 1)) * u).astype(np.float32)
    return base, q


@pytest.mark.parametrize("dim", [96, 768])
def test_non_integer_data_within_derived_tolerance(gpu_pkg, dim):
    """With S = max ||q||^2 + max ||b||^2, u = 2^-24 and gamma = dim u / (1 - dim u): two fp32 summation orders of a dot
    product differ by at most 2 gamma ||q|| ||b|| <= gamma S, the epilogue doubles that, its own roundings add at most
    4 u S.  Ids must agree wherever the oracle's neighbouring gaps exceed 4 x that."""
    rng = np.random.default_rng(7000 + dim)
    base, q = _gaussian_with_planted_neighbours(rng, 20000, 37, dim)
    with gpu_pkg.BruteForceIndex(base) as idx:
        ids, d = idx.search(q, 5)
    oi, od = oracle.search_bf(base, q, 5)
    S = float((q.astype(np.float64) ** 2).sum(1).max() + (base.astype(np.float64) ** 2).sum(1).max())
    u = 2.0 ** -24
    gamma = dim * u / (1 - dim * u)
    tol = (2 * gamma + 4 * u) * S
    print(f"dim {dim}: tol {tol:.3e}, max |d - oracle| {np.abs(d.astype(np.float64) - od).max():.3e}")
    assert np.all(np.abs(d.astype(np.float64) - od.astype(np.float64)) <= tol)
    gaps_ok = np.ones_like(oi, dtype=bool)
    od6 = np.sort(np.stack([oracle.l2_row(q[i], base) for i in range(len(q))]), axis=1)[:, :7]
    for i in range(len(q)):
        for t in range(5):
            lo = od6[i, t] - od6[i, t - 1] if t > 0 else np.inf
            hi = od6[i, t + 1] - od6[i, t]
            gaps_ok[i, t] = min(lo, hi) > 4 * tol
    assert gaps_ok.mean() > 0.9
    assert np.array_equal(ids[gaps_ok], oi[gaps_ok])
    # and bit for bit what the chain order gives (the kernel's own order; no two of a query's distances are equal here)
    ci, cd = oracle.search_bf(base, q, 5, dot_order="chain")
    assert np.array_equal(d.view(np.int32), cd.view(np.int32)) and np.array_equal(ids, ci)


_FORCE_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
rng = np.random.default_rng(8000)
base = rng.integers(0, 219, size=(150000, 128)).astype(np.float32)
q = rng.integers(0, 219, size=(300, 128)).astype(np.float32)
base[:3000] = base[70000:73000]
base[-3000:] = base[80000:83000]
q[:4] = base[70000:70004]
with pkg.BruteForceIndex(base) as idx:
    i5, d5 = idx.search(q, 5)
    i100, d100 = idx.search_topk(q, 100)
np.savez(sys.argv[2], i5=i5, d5=d5, i100=i100, d100=d100)
print("FORCE_OK")
"""


def test_general_kernel_equals_specialised_paths_at_128(gpu_pkg, tmp_path):
    """VSEARCH_ND_FORCE=1 (read when the library is loaded, hence the subprocesses) makes vs_bf_create build a general index
    at dim 128: ids and distances of scan_nd_kernel's paths equal those of the specialised 128-d paths."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for tag, force in (("default", "0"), ("forced", "1")):
        e = dict(os.environ)
        e["VSEARCH_ND_FORCE"] = force
        path = str(tmp_path / f"{tag}.npz")
        r = subprocess.run([sys.executable, "-c", _FORCE_SCRIPT, root, path], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "FORCE_OK" in r.stdout, (tag, r.stdout[-400:], r.stderr[-1200:])
        out[tag] = np.load(path)
    for key in ("i5", "d5", "i100", "d100"):
        assert np.array_equal(out["default"][key], out["forced"][key]), key


def test_refusals_and_the_128_index_of_create_nd(gpu_pkg):
    L = gpu_pkg.lib()
    rng = np.random.default_rng(9000)
    base = rng.integers(0, 100, size=(2000, 300)).astype(np.float32)
    bp = base.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(None)
    assert L.vs_bf_create_nd(bp, 2000, 0, 0, 0, 0, C.byref(h)) == -1
    assert L.vs_bf_create_nd(bp, 200, 2049, 0, 0, 0, C.byref(h)) == -5
    assert L.vs_bf_create(bp, 2000, 64, 0, 0, 0, C.byref(h)) == -5
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.set_precision(0)
        idx.set_precision(1)
        with pytest.raises(gpu_pkg.VSearchError) as e:
            idx.set_precision(2)
        assert e.value.status == -5
        q = base[:3].copy()
        with pytest.raises(gpu_pkg.VSearchError) as e:
            gpu_pkg.BruteForceIndex.search_vshards([idx], q, 5)
        assert e.value.status == -5 and "300" in str(e.value)
        ids = np.zeros((3, 5), dtype=np.int32)
        d = np.zeros((3, 5), dtype=np.float32)
        assert L.vs_ivf_search(idx._h, q.ctypes.data_as(C.c_void_p), 3, 5, 4, ids.ctypes.data_as(C.c_void_p),
                               d.ctypes.data_as(C.c_void_p), None, None) == -5
        # still usable after the refusals
        oi, od = oracle.search_bf(base, q, 5)
        gi, gd = idx.search(q, 5)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od)
    # vs_bf_create_nd at 128 is vs_bf_create: same results, same launches
    b128 = gpu_pkg.synth_sift(40000, seed=21)
    q128 = gpu_pkg.synth_sift(100, seed=22)
    res = []
    for create in (L.vs_bf_create, L.vs_bf_create_nd):
        hh = C.c_void_p(None)
        assert create(b128.ctypes.data_as(C.c_void_p), 40000, 128, 0, 0, 0, C.byref(hh)) == 0
        ids = np.zeros((100, 5), dtype=np.int32)
        d = np.zeros((100, 5), dtype=np.float32)
        assert L.vs_prof_enable(hh, 1) == 0
        assert L.vs_set_precision(hh, 2) == 0  # the int8 copy exists on both
        assert L.vs_set_precision(hh, 0) == 0
        assert L.vs_bf_search(hh, q128.ctypes.data_as(C.c_void_p), 100, 5, ids.ctypes.data_as(C.c_void_p),
                              d.ctypes.data_as(C.c_void_p), None) == 0
        ms, n = C.c_double(0), C.c_int64(0)
        assert L.vs_prof_read(hh, 0, C.byref(ms), C.byref(n)) == 0
        assert L.vs_index_dim(hh) == 128
        res.append((ids, d, n.value))
        L.vs_destroy(hh)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2] > 0
    oi, od = oracle.search_bf(b128, q128, 5)
    assert np.array_equal(res[1][0], oi) and np.array_equal(res[1][1], od)


def test_cli_at_dim_300(gpu_pkg, tmp_path):
    rng = np.random.default_rng(9500)
    base, q = _int_data(rng, 5000, 50, 300)
    gpu_pkg.write_fvecs(str(tmp_path / "base.fvecs"), base)
    gpu_pkg.write_fvecs(str(tmp_path / "query.fvecs"), q)
    exe = os.path.join(os.path.dirname(gpu_pkg.LIB_PATH), "vsearch_bf")
    assert os.path.exists(exe), "vsearch_bf not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = gpu_pkg.hip_runtime_dir() + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, "base.fvecs", "query.fvecs", "5", "results.txt"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gi, gd = oracle.parse_results_txt(str(tmp_path / "results.txt"))
    oi, od = oracle.search_bf(base, q, 5)
    assert np.array_equal(gi, oi)
    # (results.txt carries six significant digits: the oracle's distances go through the same format)
    oracle.write_results(str(tmp_path / "oracle_results.txt"), oi, od)
    wi, wd = oracle.parse_results_txt(str(tmp_path / "oracle_results.txt"))
    assert np.array_equal(gi, wi) and np.array_equal(gd, wd)
    assert open(tmp_path / "results.txt").read() == open(tmp_path / "oracle_results.txt").read()
    metrics = [f for f in os.listdir(tmp_path) if f.endswith("metrics.txt")]
    text = r.stdout + "".join(open(tmp_path / f).read() for f in metrics)
    assert "Dimension: 300" in text


def test_long_one_million_rows_at_dim_960(gpu_pkg):
    """The one long test of this file: the GIST-1M shape, 1 000 000 x 960 (3.84 GB on the host), integer data in [0, 94),
    64 queries, k = 5, against the oracle (about a minute of CPU on 16 threads)."""
    rng = np.random.default_rng(9900)
    n, dim = 1000000, 960
    base = np.empty((n, dim), dtype=np.float32)
    for r0 in range(0, n, 50000):
        base[r0:r0 + 50000] = rng.integers(0, _hi(dim), size=(50000, dim), dtype=np.int32)
    q = rng.integers(0, _hi(dim), size=(64, dim)).astype(np.float32)
    base[:25000] = base[400000:425000]
    base[-25000:] = base[500000:525000]
    q[:4] = base[400000:400004]
    _check_exact(gpu_pkg, base, q, (5,))
