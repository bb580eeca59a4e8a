"""The float16 brute-force index (BruteForceIndex.from_f16, vs_bf_create_nd_f16): every call returns what it
returns on the rows widened to float -- checked against the CPU oracles (integer data: oracle.search_bf; real-valued
data: the chain oracle's bits, as tests/test_gpu_cancel.py; inner product: the exact integer product, as
tests/test_gpu_ip.py) and, for the device calls, against the widened fp32 index in the same process, bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
from cancel_data import bits, sorted_scores  # noqa: E402
from test_gpu_cancel import _assert_same, _bf_dev, _flags  # noqa: E402
from test_gpu_ip import _ip_reference, _tie_flags  # noqa: E402
from test_gpu_nd import _hi, _int_data  # noqa: E402

pytestmark = pytest.mark.gpu

N = 4099  # no multiple of 64: the last block runs into the spare rows


@functools.lru_cache(maxsize=None)
def _ints(dim, n=N, nq=70):
    """integers below min(256, _hi(dim)), all exact in float16, with duplicate rows and queries that are duplicated rows"""
    rng = np.random.default_rng(16000 + dim + n)
    base, q = _int_data(rng, n, nq, dim, hi=min(256, _hi(dim)), dup=0.05)
    if n >= 2:
        base[n - 1] = base[0]
        q[0] = base[0]
    assert np.array_equal(base.astype(np.float16).astype(np.float32), base)
    return base.astype(np.float16), q


@functools.lru_cache(maxsize=None)
def _reals(dim, nq=70):
    """gaussian rows rounded to float16 with planted subnormals, negative values, values near 6e4 and duplicate rows;
    fp32 queries that are not rounded, the first 16 of them rows of the base (their best distances cancel)"""
    rng = np.random.default_rng(17000 + dim)
    base = rng.normal(0, 1, size=(N, dim)).astype(np.float16)
    sub = np.array([1, 2, 0x3FF, 0x8001, 0x83FF], dtype=np.uint16).view(np.float16)  # subnormals of both signs
    base[rng.integers(0, N, 400), rng.integers(0, dim, 400)] = sub[rng.integers(0, len(sub), 400)]
    base[5, :] = sub[np.arange(dim) % len(sub)]  # a row of nothing else
    base[rng.integers(0, N, 6), rng.integers(0, dim, 6)] = np.float16(6.0e4) * np.array([1, -1, 1, -1, 1, -1], dtype=np.float16)
    base[N - 200:] = base[100:300]  # duplicate rows
    base[1000:1003] = base[7]
    q = rng.normal(0, 1, size=(nq, dim)).astype(np.float32)
    q[:16] = base[[7, 100, 150, 299, 5, 64, 4098, 63] + list(range(2000, 2008))].astype(np.float32)
    return base, q


@pytest.mark.parametrize("dim", [1, 3, 31, 32, 33, 100, 128, 130, 768, 2048])
def test_integer_data_equals_the_oracle(gpu_pkg, dim):
    base, q = _ints(dim)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        assert idx.getDim() == dim and idx.getNumDocs() == N
        for k in (1, 5, 15):
            oi, od = oracle.search_bf(base.astype(np.float32), q, k)
            tm = gpu_pkg.Timing()
            ids, d = idx.search(q, k, tm)
            assert np.array_equal(bits(d), bits(od)) and np.array_equal(ids, oi), (dim, k)
            assert tm.tie_queries > 0, (dim, k)


@pytest.mark.parametrize("n", [1, 17])
def test_tiny_bases_at_dim_100(gpu_pkg, n):
    base, q = _ints(100, n, 33)
    oi, od = oracle.search_bf(base.astype(np.float32), q, 1)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        ids, d = idx.search(q, 1)
    assert np.array_equal(bits(d), bits(od)) and np.array_equal(ids, oi)


@pytest.mark.parametrize("dim", [33, 384, 1024])
def test_real_valued_half_rows_equal_the_chain_oracle(gpu_pkg, dim):
    base, q = _reals(dim)
    b32 = base.astype(np.float32)
    raw = base.view(np.uint16)
    assert (((raw & 0x7C00) == 0) & ((raw & 0x03FF) != 0)).sum() >= 100, "float16 subnormals are present"
    assert (b32 < 0).any() and (np.abs(b32) > 5.9e4).any()
    ri, rd = sorted_scores(q, b32, 16)
    assert (rd[:16, 0] <= 0).any() or (rd[:16, 0] == rd[:16, 1]).any(), "self-queries cancel or tie"
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        for k in (5, 15):
            wi, wd = oracle.search_bf(b32, q, k, dot_order="chain")
            _assert_same(idx.search(q, k), (wi, wd), ("f16 host", dim, k))
            for nb, B in ((2, 32), (4, 17)):
                gi, gd, fl = _bf_dev(idx, q, nb, B, k)
                _assert_same((gi, gd), (ri[:nb * B, :k + 1], rd[:nb * B, :k + 1]), ("f16 dev", dim, nb, B, k))
                assert np.array_equal(fl, _flags(rd[:nb * B, :k + 1])), (dim, nb, B, k)


@pytest.mark.parametrize("dim", [33, 768])
def test_inner_product_equals_the_exact_integer_product(gpu_pkg, dim):
    rng = np.random.default_rng(18000 + dim)
    base = rng.integers(-20, 21, size=(N, dim)).astype(np.float32)
    q = rng.integers(-20, 21, size=(64, dim)).astype(np.float32)
    base[N - 300:] = base[:300]
    base[:, :2] = -1.0 - np.abs(base[:, :2])
    q[3] = 0.0
    q[3, :2] = (5.0, 7.0)  # negative products with every row but the planted ones, orthogonal to it: exactly zero, the best
    base[[11, 2048, N - 1], :2] = 0.0
    k = 5
    wi, wd = _ip_reference(q, base, k + 1)
    assert (wd == 0).any()
    with gpu_pkg.BruteForceIndex.from_f16(base.astype(np.float16), metric=gpu_pkg.METRIC_IP) as idx:
        gi, gd, fl = _bf_dev(idx, q, 2, 32, k)
        hi_, hd = idx.search(q, k)
    assert np.array_equal(gd, wd) and np.array_equal(gi, wi)
    assert np.array_equal(np.signbit(gd), np.signbit(wd) | (wd == 0)), "an exactly zero product comes back as -0.0"
    assert np.array_equal(fl, _tie_flags(wd))
    assert np.array_equal(hi_, wi[:, :k]) and np.array_equal(hd, -wd[:, :k])


@pytest.mark.parametrize("k", [16, 128])
def test_wide_k_at_dim_100(gpu_pkg, k):
    base, q = _ints(100)
    oi, od = oracle.search_bf(base.astype(np.float32), q[:40], k)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        tm = gpu_pkg.Timing()
        ids, d = idx.search_topk(q[:40], k, tm)
    assert np.array_equal(bits(d), bits(od)) and np.array_equal(ids, oi)
    assert tm.tie_queries > 0


def test_device_calls_equal_the_widened_fp32_index(gpu_pkg):
    """search_dev_multi at B = 16, 17, 32 and the score matrix, bit for bit; and no route but the per-batch one is taken"""
    import torch
    base, q = _reals(384, 128)
    n_sc, ld = len(base), 4112
    s = torch.cuda.current_stream().cuda_stream
    qd = torch.from_numpy(q[:20].copy()).cuda()
    out = {}
    with gpu_pkg.BruteForceIndex.from_f16(base) as h16, gpu_pkg.BruteForceIndex(base.astype(np.float32)) as f32:
        for name, idx in (("f16", h16), ("f32", f32)):
            sc = torch.full((20, ld), -1.0, dtype=torch.float32, device="cuda")
            idx.scores_dev(qd.data_ptr(), 20, sc.data_ptr(), ld, s)
            torch.cuda.synchronize()
            out[name] = [sc.cpu().numpy()] + [_bf_dev(idx, q, 4, B, 5) for B in (16, 17, 32)] + [_bf_dev(idx, q, 1, 16, 5, "one")]
        assert h16.one_stats() == (0, 0) and h16.filter_stats() == (0, 0, 0, 0)
        with pytest.raises(RuntimeError):
            h16.set_precision(2)
        h16.set_precision(1)
    assert np.array_equal(bits(out["f16"][0]), bits(out["f32"][0])) and np.all(out["f16"][0][:, n_sc:] == -1.0)
    for got, want in zip(out["f16"][1:], out["f32"][1:]):
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("dim", [1, 33, 2048])
def test_layout_round_trip(gpu_pkg, dim):
    base = _reals(dim)[0] if dim >= 33 else _ints(dim)[0]
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        assert np.array_equal(idx.f16_rows(0, N).view(np.uint16), base.view(np.uint16))
        assert np.array_equal(idx.f16_rows(N - 70, 70).view(np.uint16), base[N - 70:].view(np.uint16))  # ends at the last row
        with pytest.raises(RuntimeError):
            idx.f16_rows(N - 1, 2)
