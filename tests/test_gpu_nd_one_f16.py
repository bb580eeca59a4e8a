"""The single-call scan on float16 rows (scan_one_nd_f16_kernel).  Every call asserts from vs_bf_one_plan_f16
that it is on route 4 and from vs_bf_one_f16_stats that one launch per batch was counted.  Expected values are CPU
references on the widened rows, never another route of the library, except in the test of route independence."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
from cancel_data import bits, sorted_scores  # noqa: E402
from test_gpu_cancel import _assert_same, _bf_dev, _flags  # noqa: E402
from test_gpu_ip import _ip_reference  # noqa: E402
from test_gpu_nd import _int_data  # noqa: E402
from test_gpu_nd_f16 import N, _ints, _reals  # noqa: E402

pytestmark = pytest.mark.gpu


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _counted(pkg, idx, nb, B, k, call):
    """call() after asserting route 4 from the plan; the half-row counter rises by nb, vs_bf_one_stats stays (0, 0)"""
    plan = pkg.BruteForceIndex.one_plan_f16(idx.n, idx.d, _cus(), nb, B, k)
    assert plan[0] == 4, (idx.n, idx.d, nb, B, k, plan)
    before = idx.one_f16_stats()
    got = call()
    assert idx.one_f16_stats() - before == nb and idx.one_stats() == (0, 0), (before, nb, B, k)
    return got


def _dev(pkg, idx, q, nb, B, k):  # search_dev for one batch, search_dev_multi for more
    return _counted(pkg, idx, nb, B, k, lambda: _bf_dev(idx, q, nb, B, k, "one" if nb == 1 else "multi"))


def _sorted_ref(q, b32, k1, id_offset=0):
    """sorted_scores, padded with (-1, +inf) past the rows"""
    ri, rd = sorted_scores(q, b32, min(k1, len(b32)))
    pad = k1 - ri.shape[1]
    return np.pad(ri + id_offset, ((0, 0), (0, pad)), constant_values=-1), np.pad(rd, ((0, 0), (0, pad)), constant_values=np.inf)


def _check_dev(got, ref, n, k, tag):
    gi, gd, fl = got
    _assert_same((gi, gd), (ref[0][:n, :k + 1], ref[1][:n, :k + 1]), tag)
    assert np.array_equal(fl, _flags(ref[1][:n, :k + 1])), (tag, "flags")


@pytest.mark.parametrize("dim", [1, 32, 33, 100, 256, 257, 2048])  # steps per unit: 1, 1, 2, 4, 8, 9, 64
def test_integer_data_against_the_oracle(gpu_pkg, dim):
    base, q = _ints(dim)
    b32 = base.astype(np.float32)
    ref = _sorted_ref(q[:16], b32, 16)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        for k in (1, 5, 15):
            oi, od = oracle.search_bf(b32, q[:16], k)
            for B in (1, 7, 16):
                ids, d = _counted(gpu_pkg, idx, 1, B, k, lambda: idx.search(q[:B], k))
                assert np.array_equal(bits(d), bits(od[:B])) and np.array_equal(ids, oi[:B]), (dim, k, B, "host")
                _check_dev(_dev(gpu_pkg, idx, q, 1, B, k), ref, B, k, (dim, k, B, "dev"))


@pytest.mark.parametrize("n", [1, 17, 63, 64, 65])  # (n = 1: the whole stream is shorter than the ring)
def test_ragged_and_tiny_bases_at_dim_100(gpu_pkg, n):
    base, q = _int_data(np.random.default_rng(19500 + n), n, 7, 100, dup=0.0)
    if n >= 2:
        base[n - 1] = q[0] = base[0]  # a tie at distance 0
    off = 1000 if n == 65 else 0  # (id_offset != 0 once)
    ref = _sorted_ref(q, base, 6, id_offset=off)
    assert n > 5 or (ref[0][:, n:] == -1).all()
    with gpu_pkg.BruteForceIndex.from_f16(base.astype(np.float16), id_offset=off) as idx:
        _check_dev(_dev(gpu_pkg, idx, q, 1, 7, 5), ref, 7, 5, n)


def test_every_wave_works_several_units(gpu_pkg):
    """three complete runs of units (checkpoints, bounded insertion, the ring across unit boundaries), and two and 70
    rows; two consecutive calls each: both walk directions"""
    k, B = 15, 16
    grid, unit = gpu_pkg.BruteForceIndex.one_plan_f16(10 ** 7, 20, _cus(), 1, B, k)[1:3]
    run = grid * 8 * unit
    for n in (3 * run, 2 * run + 70):
        assert gpu_pkg.BruteForceIndex.one_plan_f16(n, 20, _cus(), 1, B, k)[1:] == (grid, 64, 3)
        base, q = _int_data(np.random.default_rng(19000 + n % 1000), n, B, 20)
        ref = _sorted_ref(q, base, k + 1)
        with gpu_pkg.BruteForceIndex.from_f16(base.astype(np.float16)) as idx:
            for rep in range(2):
                _check_dev(_dev(gpu_pkg, idx, q, 1, B, k), ref, B, k, (n, rep))


@pytest.mark.parametrize("dim", [33, 384])
def test_real_valued_half_rows_equal_the_chain_oracle(gpu_pkg, dim):
    """planted subnormals, values near 6e4, duplicate rows and self-queries whose best distances cancel"""
    base, q = _reals(dim)
    ref = sorted_scores(q[:48], base.astype(np.float32), 16)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        for k in (5, 15):
            for nb, B in ((1, 1), (1, 16), (3, 16), (2, 7)):
                _check_dev(_dev(gpu_pkg, idx, q, nb, B, k), ref, nb * B, k, (dim, nb, B, k))


@pytest.mark.parametrize("dim", [33, 768])
def test_inner_product_equals_the_exact_integer_product(gpu_pkg, dim):
    rng = np.random.default_rng(18000 + dim)
    base = rng.integers(-20, 21, size=(N, dim)).astype(np.float32)
    q = rng.integers(-20, 21, size=(48, dim)).astype(np.float32)
    base[N - 300:] = base[:300]
    base[:, :2] = -1.0 - np.abs(base[:, :2])
    q[3] = 0.0
    q[3, :2] = (5.0, 7.0)  # negative products with every row but the planted ones: exactly zero there, the best
    base[[11, 2048, N - 1], :2] = 0.0
    with gpu_pkg.BruteForceIndex.from_f16(base.astype(np.float16), metric=gpu_pkg.METRIC_IP) as idx:
        for k in (5, 15):
            wi, wd = _ip_reference(q, base, k + 1)
            assert (wd[3] == 0).any()
            gi, gd, fl = _dev(gpu_pkg, idx, q, 3, 16, k)
            assert np.array_equal(gd, wd) and np.array_equal(gi, wi), (dim, k)
            assert np.array_equal(np.signbit(gd), np.signbit(wd) | (wd == 0)), "an exactly zero product comes back as -0.0"
            assert np.array_equal(fl, _flags(wd))


def test_results_do_not_depend_on_the_route(gpu_pkg):
    """the same 48 queries as 3 batches of 16 (route 4) and inside a 4-batch call (the per-batch kernel), one index"""
    base, q = _reals(384)
    assert gpu_pkg.BruteForceIndex.one_plan_f16(N, 384, _cus(), 4, 16, 5) == (0, 0, 0, 0)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        one = _dev(gpu_pkg, idx, q, 3, 16, 5)
        per = _bf_dev(idx, q, 4, 16, 5)
        assert idx.one_f16_stats() == 3, "the 4-batch call took no single-call launch"
    assert np.array_equal(one[0], per[0][:48]) and np.array_equal(bits(one[1]), bits(per[1][:48])) and np.array_equal(one[2], per[2][:48])
