"""Brute force for k up to 128 (vs_bf_search_topk, vs_bf_search_topk_dev_multi) against the CPU oracle and exact
integer distances.  Integer-valued data: ids and distances bit for bit.  For k >= 16 the tie order is the oracle's:
select_topk's slots, stably sorted."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def _int_data(rng, n, nq, hi=219):
    return (rng.integers(0, hi, size=(n, 128)).astype(np.float32),
            rng.integers(0, hi, size=(nq, 128)).astype(np.float32))


def _check_exact(pkg, base, q, k, precisions=(1, 0), id_offset=0):
    oi, od = oracle.search_bf(base, q, k)
    oi = np.where(oi >= 0, oi + id_offset, oi)
    with pkg.BruteForceIndex(base, id_offset=id_offset) as idx:
        for precision in precisions:
            idx.set_precision(precision)
            ids, d = idx.search_topk(q, k)
            assert np.array_equal(ids, oi), f"ids differ (N={len(base)}, nq={len(q)}, k={k}, precision={precision})"
            assert np.array_equal(d, od), f"dists differ (N={len(base)}, k={k}, precision={precision})"


def _exact_sorted(q, base, k1, id_offset=0):
    """k1 best by (dist, id) per query from exact integer distances (float64 products of integers < 2^53 are exact)."""
    b64 = base.astype(np.float64)
    bn = (b64 ** 2).sum(1)
    out_i = np.full((len(q), k1), -1, dtype=np.int64)
    out_d = np.full((len(q), k1), np.inf)
    for c0 in range(0, len(q), 32):
        qq = q[c0:c0 + 32].astype(np.float64)
        d = (qq ** 2).sum(1)[:, None] + bn[None, :] - 2.0 * (qq @ b64.T)
        m = min(k1, base.shape[0])
        for r in range(len(qq)):
            cand = np.argpartition(d[r], m - 1)[:m] if m < base.shape[0] else np.arange(base.shape[0])
            kth = d[r, cand].max()
            cand = np.nonzero(d[r] <= kth)[0]  # every row at the k1-th distance, so that (dist, id) picks the right ones
            o = np.lexsort((cand, d[r, cand]))[:m]
            out_i[c0 + r, :m] = cand[o] + id_offset
            out_d[c0 + r, :m] = d[r, cand[o]]
    return out_i.astype(np.int32), out_d.astype(np.float32)


def _dev_multi(pkg, idx, q, n_batches, B, k):
    import torch
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(np.ascontiguousarray(q[:n_batches * B])).to(dev)
    oi = torch.full((n_batches * B, k + 1), -7, dtype=torch.int32, device=dev)
    od = torch.zeros((n_batches * B, k + 1), dtype=torch.float32, device=dev)
    fl = torch.full((n_batches * B,), -7, dtype=torch.int32, device=dev)
    idx.search_topk_dev_multi(qd.data_ptr(), n_batches, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()


def _adjacent_equal(d):
    f = np.isfinite(d[:, :-1]) & (d[:, :-1] == d[:, 1:])
    return f.any(1).astype(np.int32)


@pytest.mark.parametrize("k", [16, 17, 31, 32, 33, 64, 100, 127, 128])
def test_k_grid_exact(gpu_pkg, k):
    rng = np.random.default_rng(300 + k)
    base, q = _int_data(rng, 6000, 33)
    _check_exact(gpu_pkg, base, q, k)


def test_k_up_to_15_is_search(gpu_pkg):
    rng = np.random.default_rng(9)
    base, q = _int_data(rng, 6000, 40, hi=8)  # small alphabet: ties, so the replay runs too
    with gpu_pkg.BruteForceIndex(base) as idx:
        for k in (1, 5, 15):
            a = idx.search(q, k)
            b = idx.search_topk(q, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n", [1, 17, 100, 127, 129, 4099])
def test_small_and_ragged_bases(gpu_pkg, n):
    rng = np.random.default_rng(400 + n)
    base, q = _int_data(rng, n, 7)
    oi, od = oracle.search_bf(base, q, 100)
    with gpu_pkg.BruteForceIndex(base) as idx:
        ids, d = idx.search_topk(q, 100)
    assert np.array_equal(ids, oi) and np.array_equal(d, od)
    if n < 100:
        assert (ids[:, n:] == -1).all() and np.isinf(d[:, n:]).all()


def test_ties_and_duplicates_k100(gpu_pkg):
    rng = np.random.default_rng(7)
    base = rng.integers(0, 3, size=(5000, 128)).astype(np.float32)
    base[1000:1200] = base[0:200]
    base[3000:3050] = base[0]
    q = np.concatenate([base[[0, 5, 1000, 3001]], rng.integers(0, 3, size=(20, 128)).astype(np.float32)])
    _check_exact(gpu_pkg, base, q, 100)
    same = np.tile(base[:1], (300, 1))
    _check_exact(gpu_pkg, same, q[:3], 100)
    ramp = np.zeros((4000, 128), dtype=np.float32)
    ramp[:, 0] = np.arange(4000, 0, -1) % 251
    _check_exact(gpu_pkg, ramp, np.zeros((3, 128), dtype=np.float32), 100)
    # more than one chunk of 1 024 queries and a ragged tail, on a base past the k = 100 dense prefix (53 248 rows): the
    # queries that equal a planted duplicate are flagged in every chunk
    big = rng.integers(0, 219, size=(60000, 128)).astype(np.float32)
    big[56000:56300] = big[:300]
    qb = rng.integers(0, 219, size=(2100, 128)).astype(np.float32)
    qb[::7] = big[rng.integers(0, 300, size=300)]
    _check_exact(gpu_pkg, big, qb, 100)


def test_mass_duplicates_overflow_to_dense_path(gpu_pkg):
    """20 000 copies of one row behind the prefix: the candidate lists overflow and the dense fallback answers."""
    rng = np.random.default_rng(11)
    base, q = _int_data(rng, 70000, 128)
    base[50000:70000] = base[123]
    q[:40] = base[123]
    q[40:60] = base[123] + 1
    _check_exact(gpu_pkg, base, q, 100, precisions=(1,))
    with gpu_pkg.BruteForceIndex(base) as idx:  # device form: (dist, id) order
        oi, od, fl = _dev_multi(gpu_pkg, idx, q, 4, 32, 100)
    ei, ed = _exact_sorted(q, base, 101)
    assert np.array_equal(oi, ei) and np.array_equal(od, ed)
    assert np.array_equal(fl, _adjacent_equal(ed))


@pytest.fixture(scope="module")
def sift1m(gpu_pkg):
    base = gpu_pkg.synth_sift(1_000_000, seed=21)
    q = gpu_pkg.synth_sift(128, seed=22)
    return base, q, _exact_sorted(q, base, 101)


@pytest.mark.parametrize("precision", [1, 0])
def test_sift1m_shape_k100(gpu_pkg, sift1m, precision):
    base, q, (ei, ed) = sift1m
    with gpu_pkg.BruteForceIndex(base) as idx:
        idx.set_precision(precision)
        tm = gpu_pkg.Timing()
        ids, d = idx.search_topk(q, 100, tm)
        oi, od, fl = _dev_multi(gpu_pkg, idx, q, 4, 32, 100)
    # device form: exactly the (dist, id) order
    assert np.array_equal(oi, ei) and np.array_equal(od, ed)
    assert np.array_equal(fl, _adjacent_equal(ed))
    # host call: the 100 smallest distances; each id at its own distance; select_topk's ids on a query subset
    assert np.array_equal(d, ed[:, :100])
    bn = (base.astype(np.float64) ** 2).sum(1)
    for r in range(len(q)):
        assert len(set(ids[r].tolist())) == 100
        dd = (q[r].astype(np.float64) ** 2).sum() + bn[ids[r]] - 2.0 * (base[ids[r]].astype(np.float64) @ q[r])
        assert np.array_equal(dd.astype(np.float32), d[r])
    sub = q[:32]
    o_i, o_d = oracle.search_bf(base, sub, 100)
    assert np.array_equal(ids[:32], o_i) and np.array_equal(d[:32], o_d)


@pytest.mark.parametrize("k", [16, 100, 128])
def test_device_form_grid(gpu_pkg, k):
    rng = np.random.default_rng(500 + k)
    base, q = _int_data(rng, 60000, 33 * 32, hi=40)
    ei, ed = _exact_sorted(q, base, k + 1)
    with gpu_pkg.BruteForceIndex(base) as idx:
        for B in (1, 5, 32):
            for nb in (1, 3, 33):
                oi, od, fl = _dev_multi(gpu_pkg, idx, q, nb, B, k)
                n = nb * B
                assert np.array_equal(oi, ei[:n]) and np.array_equal(od, ed[:n]), f"k={k} B={B} nb={nb}"
                assert np.array_equal(fl, _adjacent_equal(ed[:n])), f"flags k={k} B={B} nb={nb}"


def test_inner_product_and_id_offset(gpu_pkg):
    rng = np.random.default_rng(6)
    base, q = _int_data(rng, 20000, 10, hi=100)
    base[:, 0] += np.arange(20000) % 7
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP) as idx:
        ids, d = idx.search_topk(q, 64)
    s = q.astype(np.float64) @ base.astype(np.float64).T
    for r in range(len(q)):
        o = np.lexsort((np.arange(len(base)), -s[r]))[:64]
        assert np.array_equal(d[r], s[r, o].astype(np.float32))
        assert np.array_equal(ids[r], o)  # (no tie replay for IP: equal scores by id, as vs_bf_search)
    base2, q2 = _int_data(rng, 70000, 40)
    _check_exact(gpu_pkg, base2, q2, 100, precisions=(1,), id_offset=1_000_000)


def test_non_integer_data_within_tolerance(gpu_pkg):
    rng = np.random.default_rng(5)
    base = rng.normal(0, 1, size=(70000, 128)).astype(np.float32)
    q = rng.normal(0, 1, size=(37, 128)).astype(np.float32)
    k = 50
    with gpu_pkg.BruteForceIndex(base) as idx:
        ids, d = idx.search_topk(q, k)
    oi, od = oracle.search_bf(base, q, k)
    scale = float((q ** 2).sum(1).max() + (base ** 2).sum(1).max())
    tol = 2e-6 * scale
    assert np.allclose(d, od, rtol=0, atol=tol)
    od_all = np.sort(np.stack([oracle.l2_row(q[i], base) for i in range(len(q))]), axis=1)[:, :k + 2]
    gaps_ok = np.ones_like(oi, dtype=bool)
    for i in range(len(q)):
        for t in range(k):
            lo = od_all[i, t] - od_all[i, t - 1] if t > 0 else np.inf
            hi = od_all[i, t + 1] - od_all[i, t]
            gaps_ok[i, t] = min(lo, hi) > 4 * tol
    assert gaps_ok.mean() > 0.9
    assert np.array_equal(ids[gaps_ok], oi[gaps_ok])


def test_non_integer_query_on_integer_base(gpu_pkg):
    """The int8 path skips such a batch for k <= 15 (flag 2); the wide-k path scans the fp32 rows and answers directly."""
    rng = np.random.default_rng(12)
    base, q = _int_data(rng, 70000, 32)
    q[3, 7] += 0.5
    with gpu_pkg.BruteForceIndex(base) as idx:
        ids, d = idx.search_topk(q, 100)
        oi, od, fl = _dev_multi(gpu_pkg, idx, q, 1, 32, 100)
        _, _, fl5 = _dev_multi(gpu_pkg, idx, q, 1, 32, 5)
    assert (fl5 == 2).all()
    wi, wd = oracle.search_bf(base, q, 100)
    assert np.array_equal(ids, wi) and np.array_equal(d, wd)
    assert set(np.unique(fl).tolist()) <= {0, 1}
    assert np.array_equal(od[:, :100][fl == 0], wd[fl == 0])


def test_limits(gpu_pkg):
    rng = np.random.default_rng(1)
    base, q = _int_data(rng, 500, 2)
    with gpu_pkg.BruteForceIndex(base) as idx:
        for k, status in ((129, -5), (0, -1)):
            with pytest.raises(gpu_pkg.VSearchError) as e:
                idx.search_topk(q, k)
            assert e.value.status == status
        with pytest.raises(gpu_pkg.VSearchError) as e:
            idx.search(q, 16)
        assert e.value.status == -5
    shards = [gpu_pkg.BruteForceIndex(base[:250]), gpu_pkg.BruteForceIndex(base[250:], id_offset=250)]
    try:
        with pytest.raises(gpu_pkg.VSearchError) as e:
            gpu_pkg.BruteForceIndex.search_vshards(shards, q, 16)
        assert e.value.status == -5
    finally:
        for s in shards:
            s.close()


def _exe(pkg, name):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), name)
    assert os.path.exists(exe), f"{name} not built (make -C hai-25-rag-on-edge_amd/csrc all)"
    return exe


def test_cli_groundtruth_and_ivf_recall(gpu_pkg, tmp_path):
    base = gpu_pkg.synth_sift(20000, seed=31)
    q = gpu_pkg.synth_sift(50, seed=32)
    bf, qf, gt = str(tmp_path / "base.fvecs"), str(tmp_path / "q.fvecs"), str(tmp_path / "gt.ivecs")
    gpu_pkg.write_fvecs(bf, base)
    gpu_pkg.write_fvecs(qf, q)
    r = subprocess.run([_exe(gpu_pkg, "vsearch_bf"), "--groundtruth", bf, qf, gt], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = gpu_pkg.read_ivecs(gt)
    oi, _ = oracle.search_bf(base, q, 100)
    assert got.shape == (50, 100) and np.array_equal(got, oi)

    ivf, _ = gpu_pkg.IVFIndex.build(base, 32, max_iter=5, seed=42)
    idir = str(tmp_path / "index")
    with ivf:
        ivf.save(idir)
    res = str(tmp_path / "ivf_out")
    r = subprocess.run([_exe(gpu_pkg, "vsearch_ivf"), idir, qf, res, "none.so", "10", "4", gt], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Recall@10: ([0-9.eE+-]+)%", r.stdout)
    assert m, r.stdout
    pid, _ = oracle.parse_results_txt(os.path.join(res, "results.txt"))
    pid = np.array(pid)
    want = np.mean([len(set(pid[i, :10].tolist()) & set(got[i, :10].tolist())) / 10.0 for i in range(len(q))])
    assert abs(float(m.group(1)) - 100.0 * want) < 1e-3
    assert 0.0 < want <= 1.0


def test_cli_positional_k100(gpu_pkg, tmp_path):
    rng = np.random.default_rng(33)
    base, q = _int_data(rng, 20000, 40)
    bf, qf, out = str(tmp_path / "base.fvecs"), str(tmp_path / "q.fvecs"), str(tmp_path / "sift_results.txt")
    gpu_pkg.write_fvecs(bf, base)
    gpu_pkg.write_fvecs(qf, q)
    r = subprocess.run([_exe(gpu_pkg, "vsearch_bf"), bf, qf, "100", out], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    oi, od = oracle.search_bf(base, q, 100)
    want = str(tmp_path / "want.txt")
    oracle.write_results(want, oi, od)
    assert open(out).read() == open(want).read()
