"""IVF search for 17 <= k <= 128 on a general IVF index (vs_ivf_search_topk / vs_ivf_search_topk_dev_multi; the bound,
candidate-scan and ranking kernels of vs_ivf_nd_wide.hip) against the CPU oracle.

Every assertion is an equality for every query.  On the integer data of tests/test_gpu_ivf_nd.py every distance is exact
in any summation order; on N(0, 1) data the oracle runs in the kernels' summation order (dot_order="chain") and distance
BITS are compared.  Ties rank by (distance, position in vectors_reordered), as oracle.ivf_search ranks them.

What the cases reach: nprobe = 1 leaves fewer than k entries in the partial lists (an infinite bound: every list of 16
rows or more is scanned again, lists shorter than k leave (-1, +inf) tails); nprobe = 24 gives a finite bound with few
saturated pairs; a 9000-row list under an infinite bound and 8500 equal rows under a bound of 0 overflow the 8192-key
candidate list and take the exact fallback, whose distances one thread recomputes in the MFMA's order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_gpu_ivf_nd import EMPTY, N, NLIST, _gauss_index, _hi, _int_index, _nearest, _open

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _assert_same(got, want, tag):
    """ids and distance bits (and total_candidates when both carry it), per query"""
    bad = [i for i in range(len(want[0])) if not (np.array_equal(_bits(got[1][i]), _bits(want[1][i])) and np.array_equal(got[0][i], want[0][i]))]
    assert not bad, (tag, "queries differ", bad[:10], got[0][bad[0]][:8], want[0][bad[0]][:8], got[1][bad[0]][:8], want[1][bad[0]][:8])
    if len(got) > 2 and len(want) > 2:
        assert got[2] == want[2], (tag, "total_candidates", got[2], want[2])


@pytest.mark.parametrize("dim", [3, 100, 130, 384, 2048])
def test_integer_data_equals_the_oracle(gpu_pkg, dim):
    data = _int_index(dim)
    vr, cents, off, r2o, q = data
    q = q[:70]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for k, nprobe in ((17, 1), (32, 4), (100, 4), (128, NLIST)):
            want = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe)
            got = ivf.search_topk(q, k, nprobe)
            _assert_same(got, want, (dim, k, nprobe))
            assert np.array_equal(got[1], want[1])
            if nprobe == 1:  # query 4 sits on the empty list's centroid: no candidate at all
                assert np.all(got[0][4] == -1) and np.all(got[1][4] == np.inf)
            if nprobe == NLIST:
                assert got[0].min() >= 0
        # lists shorter than k: the 1-row list and the empty one
        qq = np.stack([vr[off[5]], cents[EMPTY]])
        want = oracle.ivf_search(vr, off, r2o, cents, qq, 17, 1)
        got = ivf.search_topk(qq, 17, 1)
        _assert_same(got, want, (dim, "short lists"))
        assert np.all(got[0][1] == -1) and np.all(got[1][1] == np.inf)


@pytest.mark.parametrize("dim", [20, 100, 960])
def test_non_integer_data_equals_the_chain_oracle(gpu_pkg, dim):
    """dim 100: dim_p = 112, an odd number of 16-float segments -- the half step of the candidate scan runs"""
    vr, cents, off, r2o, q, fq, _ = _gauss_index(dim)
    qq = np.concatenate([q, fq[:58]])  # 128 queries: four batches
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        for k, nprobe in ((17, 1), (64, 4), (128, NLIST)):
            want = oracle.ivf_search(vr, off, r2o, cents, qq, k, nprobe, dot_order="chain")
            _assert_same(ivf.search_topk(qq, k, nprobe), want, (dim, k, nprobe))


def test_equals_brute_force_topk(gpu_pkg):
    """nprobe = nlist: the candidates are all rows, so the result is exact search's -- bits and ids"""
    rng = np.random.default_rng(6096)
    n, dim, nlist, k = 4000, 96, 16, 100
    base = rng.normal(0, 1, size=(n, dim)).astype(np.float32)
    q = rng.normal(0, 1, size=(70, dim)).astype(np.float32)
    b64 = base.astype(np.float64)
    cen0 = b64[rng.choice(n, nlist, replace=False)]
    assign = ((b64 * b64).sum(1)[:, None] - 2 * b64 @ cen0.T + (cen0 * cen0).sum(1)[None, :]).argmin(1)
    vr, off, r2o = gpu_pkg.ivf_layout_from_assignment(base, assign, nlist)
    cents = np.stack([vr[off[c]:off[c + 1]].mean(0) if off[c + 1] > off[c] else cen0[c] for c in range(nlist)]).astype(np.float32)
    with gpu_pkg.BruteForceIndex(base) as bf:
        bf.set_precision(1)
        bi, bd = bf.search_topk(q, k)[:2]
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ids, d, total = ivf.search_topk(q, k, nlist)
    assert total == len(q) * n
    _assert_same((ids, d), (bi, bd), "brute force")


@pytest.mark.parametrize("dim", [20, 100])
def test_fallback_by_a_long_list(gpu_pkg, dim):
    """lists of 9000 / 500 / 500 rows, nprobe 1, k 17: the bound is infinite, a query nearest list 0 has 9000 candidates"""
    rng = np.random.default_rng(7100 + dim)
    n = 10000
    vr = rng.normal(0, 1, size=(n, dim)).astype(np.float32)
    off = np.array([0, 9000, 9500, 10000], dtype=np.int32)
    r2o = rng.permutation(n).astype(np.int32)
    cents = np.stack([vr[off[c]:off[c + 1]].astype(np.float64).mean(0) for c in range(3)]).astype(np.float32)
    q = rng.normal(0, 1, size=(40, dim)).astype(np.float32)
    q[:6] = cents[0] + 0.001 * rng.normal(0, 1, size=(6, dim)).astype(np.float32)
    want = oracle.ivf_search(vr, off, r2o, cents, q, 17, 1, return_probes=True, dot_order="chain")
    n0 = int((want[3][:, 0] == 0).sum())
    assert n0 >= 6 and n0 < len(q)  # some queries take the fallback, some their candidate list
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = ivf.search_topk(q, 17, 1)
        stats = ivf.nd_widek_stats()
    _assert_same(got, want[:3], (dim, "long list"))
    assert stats[2] == n0 and stats[1] == 500 and stats[0] == 500 * (len(q) - n0), stats


def test_fallback_by_duplicates(gpu_pkg):
    """8500 copies of one row in a 9000-row list and a query equal to it: the bound is 0 and 8500 rows meet it"""
    rng = np.random.default_rng(7200)
    dim, k, nlist = 20, 100, 8
    hi = _hi(dim)
    sizes = [9000] + [200] * 7
    n = sum(sizes)
    vr = rng.integers(0, hi, size=(n, dim)).astype(np.float32)
    rep = rng.integers(0, hi, size=dim).astype(np.float32)
    vr[300:8800] = rep
    assert int((vr == rep).all(1).sum()) == 8500
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    r2o = rng.permutation(n).astype(np.int32)
    cents = np.stack([np.rint(vr[off[c]:off[c + 1]].astype(np.float64).mean(0)) for c in range(nlist)]).astype(np.float32)
    q = rng.integers(0, hi, size=(5, dim)).astype(np.float32)
    q[2] = rep
    want = oracle.ivf_search(vr, off, r2o, cents, q, k, nlist)
    assert np.array_equal(want[0][2], r2o[300:400]) and np.all(want[1][2] == 0)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        got = ivf.search_topk(q, k, nlist)
        stats = ivf.nd_widek_stats()
    _assert_same(got, want, "duplicates")
    assert stats[2] >= 1, stats


def test_state_between_groups_and_calls(gpu_pkg):
    """1100 queries in one host call are two launch groups (1024 + 76); the candidate counters are left clean"""
    data = _int_index(100)
    vr, cents, off, r2o, q = data
    rng = np.random.default_rng(7300)
    qq = rng.integers(0, _hi(100), size=(1100, 100)).astype(np.float32)
    qq[:96] = q
    k, nprobe = 40, 4
    want = oracle.ivf_search(vr, off, r2o, cents, qq, k, nprobe)
    want5 = oracle.ivf_search(vr, off, r2o, cents, q, 5, nprobe)
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        assert ivf.nd_widek_stats() == (0, 0, 0)
        a = ivf.search_topk(qq, k, nprobe)
        s1 = ivf.nd_widek_stats()
        _assert_same(ivf.searchBatch(q, len(q), 5, nprobe), want5, "k 5 between two wide calls")
        b = ivf.search_topk(qq, k, nprobe)
        s2 = ivf.nd_widek_stats(reset=True)
        assert ivf.nd_widek_stats() == (0, 0, 0)
    _assert_same(a, want, "first call")
    _assert_same(b, a, "second call")
    assert s1[0] >= s1[1] > 0 and s1[2] == 0 and s2 == (2 * s1[0], s1[1], 0), (s1, s2)  # (the k 5 call counts nothing)


def test_device_call(gpu_pkg):
    """search_topk_dev_multi on a non-default torch stream: 3 batches of 24"""
    import torch
    dev = torch.device("cuda:0")
    vr, cents, off, r2o, q = _int_index(100)
    dim, nprobe, nb, B = 100, 4, 3, 24
    q = np.array(q[:nb * B])
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        st = torch.cuda.Stream()
        out = {}
        for k in (40, 5):
            with torch.cuda.stream(st):
                qd = torch.from_numpy(q).to(dev)
                gi = torch.full((nb * B, k), -7, dtype=torch.int32, device=dev)
                gd = torch.zeros((nb * B, k), dtype=torch.float32, device=dev)
                ivf.search_topk_dev_multi(qd.data_ptr(), nb, B, k, nprobe, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
            st.synchronize()
            out[k] = (gi.cpu().numpy(), gd.cpu().numpy())
        _assert_same(out[40], ivf.search_topk(q, 40, nprobe), "device call, k 40")
        _assert_same(out[40], oracle.ivf_search(vr, off, r2o, cents, q, 40, nprobe), "device call against the oracle")
        with torch.cuda.stream(st):
            gi = torch.full((nb * B, 5), -7, dtype=torch.int32, device=dev)
            gd = torch.zeros((nb * B, 5), dtype=torch.float32, device=dev)
            ivf.search_dev_multi(qd.data_ptr(), nb, B, 5, nprobe, gi.data_ptr(), gd.data_ptr(), st.cuda_stream)
        st.synchronize()
        _assert_same(out[5], (gi.cpu().numpy(), gd.cpu().numpy()), "device call, k 5")


def test_byte_index(gpu_pkg):
    """wide k on a from_u8 index scans the fp32 rows: the byte plan gets no pair"""
    data = _int_index(100)
    vr, cents, off, r2o, q = data
    q = q[:70]
    u8 = vr.astype(np.uint8)
    assert np.array_equal(u8.astype(np.float32), vr)
    with gpu_pkg.IVFIndex.from_u8(u8, cents, off, r2o) as ivf:
        ivf.searchBatch(q, len(q), 5, 4)
        before = ivf.nd_u8_stats()
        assert before[0] > 0
        for nprobe in (4, NLIST):
            _assert_same(ivf.search_topk(q, 100, nprobe), oracle.ivf_search(vr, off, r2o, cents, q, 100, nprobe), ("u8", nprobe))
        assert ivf.nd_u8_stats()[0] == before[0]
        _assert_same(ivf.searchBatch(q, len(q), 5, 4), oracle.ivf_search(vr, off, r2o, cents, q, 5, 4), "u8, k 5 afterwards")


_SIFT_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
import oracle
pkg = ge.load_package()
base = pkg.synth_sift(20000, seed=31)
q = pkg.synth_sift(70, seed=32)
cents = base[:: len(base) // 64][:64].copy()
b, c = base.astype(np.int64), cents.astype(np.int64)
assign = ((b * b).sum(1)[:, None] - 2 * (b @ c.T) + (c * c).sum(1)[None, :]).argmin(1)
vr, off, r2o = pkg.ivf_layout_from_assignment(base, assign, 64)
with pkg.IVFIndex(vectors_reordered=vr, centroids=cents, cluster_offsets=off, reorder_to_original=r2o) as ivf:
    general = pkg.lib().vs_set_precision(ivf._h, 2) == -5 and b"dim = 128" in pkg.lib().vs_last_error()
    ivf.set_precision(1)
    ti, td, tt = ivf.search_topk(q, 100, 8)
    if general:
        si, sd, st = oracle.ivf_search(vr, off, r2o, cents, q, 100, 8)
    else:
        si, sd, st = ivf.searchBatch(q, len(q), 100, 8)
np.savez(sys.argv[2], general=general, same=np.array_equal(ti, si) and np.array_equal(td, sd) and tt == st, full=ti.min() >= 0)
print("SIFT_OK")
"""


@pytest.mark.parametrize("force", [None, "1"])
def test_128d(gpu_pkg, tmp_path, force):
    """the specialised 128-d index: search_topk at k 100 is searchBatch at k 100; with VSEARCH_IVF_ND_FORCE=1 (read when an
    index is created) the general pipeline runs at dim 128 and equals the oracle (synth_sift rows: everything exact)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.pop("VSEARCH_IVF_ND_FORCE", None)
    if force:
        e["VSEARCH_IVF_ND_FORCE"] = force
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", _SIFT_SCRIPT, root, path], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SIFT_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1200:])
    out = np.load(path)
    assert bool(out["general"]) == bool(force)
    assert out["same"] and out["full"]


def test_errors(gpu_pkg):
    L = gpu_pkg.lib()
    data = _int_index(100)
    vr, cents, off, r2o, q = data
    q = np.array(q[:8])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ids = np.zeros((8, 129), dtype=np.int32)
    d = np.zeros((8, 129), dtype=np.float32)
    out3 = (C.c_int64 * 3)()
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        assert L.vs_ivf_search_topk(ivf._h, p(q), 8, 0, 4, p(ids), p(d), None, None) == -1
        assert L.vs_ivf_search_topk(ivf._h, p(q), 8, 129, 4, p(ids), p(d), None, None) == -5
        assert L.vs_ivf_search_topk_dev_multi(ivf._h, p(q), 1, 8, 0, 4, p(ids), p(d), None) == -1  # (refused before any pointer is used)
        assert L.vs_ivf_search_topk_dev_multi(ivf._h, p(q), 1, 8, 129, 4, p(ids), p(d), None) == -5
        with pytest.raises(gpu_pkg.VSearchError) as e:
            ivf.search_topk(q, 129, 4)
        assert e.value.status == -5
        _assert_same(ivf.search_topk(q, 100, 4), oracle.ivf_search(vr, off, r2o, cents, q, 100, 4), "after the refusals")
        _assert_same(ivf.search_topk(q, 5, 4), oracle.ivf_search(vr, off, r2o, cents, q, 5, 4), "k 5 through the new call")
    with gpu_pkg.BruteForceIndex(np.ascontiguousarray(vr[:500])) as bf:
        assert L.vs_ivf_search_topk(bf._h, p(q), 8, 100, 4, p(ids), p(d), None, None) == -5
        assert L.vs_ivf_search_topk_dev_multi(bf._h, p(q), 1, 8, 100, 4, p(ids), p(d), None) == -5
        assert L.vs_ivf_nd_widek_stats(bf._h, out3, 0) == -1
        bi, bd = bf.search(q, 5)
        assert bi.shape == (8, 5) and bi.min() >= 0  # still usable


def test_cli_at_dim_100(gpu_pkg, tmp_path):
    """vsearch_ivf calls the _topk host entry: top_k 40 on a saved 100-d index (batch 1: launch groups of 32 single queries)"""
    vr, cents, off, r2o, q = _int_index(100)
    q = np.array(q[:40])
    idir, qf, res = str(tmp_path / "index"), str(tmp_path / "q.fvecs"), str(tmp_path / "out")
    with _open(gpu_pkg, vr, cents, off, r2o) as ivf:
        ivf.save(idir)
    gpu_pkg.write_fvecs(qf, q)
    exe = os.path.join(os.path.dirname(gpu_pkg.LIB_PATH), "vsearch_ivf")
    assert os.path.exists(exe), "vsearch_ivf not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = gpu_pkg.hip_runtime_dir() + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe, idir, qf, res, "none.so", "40", "4"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    pid, _ = oracle.parse_results_txt(os.path.join(res, "results.txt"))
    want = oracle.ivf_search(vr, off, r2o, cents, q, 40, 4)[0]
    assert len(pid) == len(q)
    for i in range(len(q)):
        assert pid[i] == [int(x) for x in want[i] if x >= 0], i
