"""The single-call byte scan of a general index made from uint8 rows (scan_one_nd_i8_kernel): short device
calls -- fewer than 4 batches of at most 16 queries, k <= 15 -- on the byte rows of a from_u8 index are ONE launch per batch.

Every case asserts first, through vs_bf_one_plan_u8 with the device's CU count, that its call is on route 3, and then that
the index's counter of single-call launches on the byte rows (vs_bf_one_stats) rose by exactly the number of batches
while the counter of the fp32 rows did not move: results alone cannot show the route, they are the per-batch scan's.

The measured exception of the rule (at dim <= 128 a batch of more than 12 queries keeps the per-batch route,
which was 2 - 3 % faster there) takes the 16-query shapes at those dimensions off route 3.  Those shapes stay in every
case, with the same expectations of the results, and the case asserts that the plan says 0 for exactly that reason and
that no single-call launch was counted; the same case then makes the call with 12 queries per batch on route 3.

Expected values: oracle.search_bf / oracle.l2_row on nd_u8_data.u8_data (exact: every squared norm < 2^23), the int64
product of nd_u8_ip_data under inner product.  Never another route of the library, except in the test of route
independence."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import nd_one_u8_child  # noqa: E402
import nd_u8_ip_data as D  # noqa: E402
import oracle  # noqa: E402
import test_gpu_cancel as tc  # noqa: E402
from cancel_data import bits  # noqa: E402
from nd_u8_data import sqnorm_max, u8_data  # noqa: E402
from test_gpu_nd_one import KS, SHAPES, _check_int, _cus, _same_bits, _sorted_int_ref  # noqa: E402
from test_gpu_ivf_nd import _open as _open_ivf  # noqa: E402
from test_gpu_nd_u8 import _with_sqnorm  # noqa: E402

pytestmark = pytest.mark.gpu


def _f32(a):
    return a.astype(np.float32)


def _on_route_3(pkg, n, dim, nb, B, k):
    plan = pkg.BruteForceIndex.one_plan_u8(n, dim, _cus(), nb, B, k)
    assert plan[0] == 3, (n, dim, nb, B, k, plan)
    return plan


def _excepted(dim, B):
    return dim <= 128 and B > 12


def _shapes(dim):
    """SHAPES, and where their 16-query shapes fall under the measured exception the same with 12 queries"""
    return SHAPES + ((("one", 1, 12), ("multi", 3, 12)) if _excepted(dim, 16) else ())


def _call(pkg, idx, q, nb, B, k, call, byte_launches=None):
    """tc._bf_dev after asserting route 3 from the plan (route 0 exactly under the measured exception); the byte counter
    rises by nb (by 0 there; or by byte_launches), the fp32 one stays"""
    if byte_launches is None:
        if _excepted(idx.d, B):
            assert pkg.BruteForceIndex.one_plan_u8(idx.n, idx.d, _cus(), nb, B, k) == (0, 0, 0, 0)
            _on_route_3(pkg, idx.n, idx.d, nb, 12, k)
            byte_launches = 0
        else:
            _on_route_3(pkg, idx.n, idx.d, nb, B, k)
            byte_launches = nb
    before = idx.one_stats()
    got = tc._bf_dev(idx, q, nb, B, k, call)
    after = idx.one_stats()
    assert after[1] - before[1] == byte_launches, (before, after, nb, B, k, call)
    assert after[0] == before[0], (before, after)
    return got


# ---------------------------------------------------------------------------------------------------- every step shape
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 129, 192, 320, 960, 2048])  # dim_b / 64 = 1, 1, 1, 2, 3, 3, 5, 15, 32
def test_every_step_shape_against_the_oracle(gpu_pkg, dim):
    rng = np.random.default_rng(21000 + dim)
    n = 20000
    base_u8, q_u8 = u8_data(rng, n, 48, dim)
    base, q = _f32(base_u8), _f32(q_u8)
    seen = set()
    sref = _sorted_int_ref(base, q, 17)
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
        for k in KS:
            oi, od = oracle.search_bf(base, q, k + 1)
            for call, nb, B in _shapes(dim):
                fl = _check_int(_call(gpu_pkg, idx, q, nb, B, k, call), oi[:nb * B], od[:nb * B], sref, (dim, k, call, nb, B))
                seen |= set(fl.tolist())
    assert seen == ({0, 1} if dim > 1 else {1})  # (256 values of one coordinate in 20 000 rows: every query ties)


@pytest.mark.parametrize("dim", [100, 960])
@pytest.mark.parametrize("n", [1, 5, 17, 63, 64, 65, 4099])
def test_ragged_bases(gpu_pkg, dim, n):
    rng = np.random.default_rng(22000 + dim + n)
    base_u8, q_u8 = u8_data(rng, n, 7, dim, dup=0.05 if n > 1000 else 0.0)
    if n >= 2:
        base_u8[n - 1] = base_u8[0]
        q_u8[0] = base_u8[0]
    base, q = _f32(base_u8), _f32(q_u8)
    k = 5
    wi, wd = _sorted_int_ref(base, q, k + 1)
    assert (n > k) or ((wi[:, n:] == -1).all() and np.isposinf(wd[:, n:]).all())
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
        gi, gd, fl = _call(gpu_pkg, idx, q, 1, 7, k, "one")
    assert np.array_equal(gd, wd), (n, dim)
    want_fl = (np.isfinite(wd[:, 1:]) & (wd[:, 1:] == wd[:, :-1])).any(1)
    assert np.array_equal(fl != 0, want_fl) and set(np.unique(fl)) <= {0, 1}
    assert np.array_equal(gi, wi)  # ((distance, id) order: equal also where a flag is set)
    assert n < 2 or fl[0] == 1     # the planted tie on query 0


def test_every_wave_works_several_units(gpu_pkg):
    """dim 20, B = 16, k = 15 on a base of three complete runs of units (every wave works three: the checkpoints and the
    bounded insertion are in use, and the ring runs across unit boundaries) and on one of two complete runs and 70 rows.
    Two consecutive calls each: both directions.  B = 16 at dim 20 is under the measured exception (the per-batch route);
    B = 12 is the widest batch on route 3 there."""
    k, B = 15, 16
    grid, unit = gpu_pkg.BruteForceIndex.one_plan_u8(10 ** 7, 20, _cus(), 1, 12, k)[1:3]
    run = grid * 8 * unit
    for n, tag in ((3 * run, "complete"), (2 * run + 70, "incomplete")):
        plan = _on_route_3(gpu_pkg, n, 20, 1, 12, k)
        assert plan[1] == grid and plan[3] == 3, plan
        rng = np.random.default_rng(23000 + (n % 1000))
        base_u8, q_u8 = u8_data(rng, n, B, 20)
        base, q = _f32(base_u8), _f32(q_u8)
        oi, od = oracle.search_bf(base, q, k + 1)
        sref = _sorted_int_ref(base, q, k + 2)
        with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
            for rep in range(2):
                fl = _check_int(_call(gpu_pkg, idx, q, 1, B, k, "one"), oi, od, sref, (tag, rep))
                f12 = _check_int(_call(gpu_pkg, idx, q, 1, 12, k, "one"), oi[:12], od[:12], sref, (tag, rep, 12))
        assert set(fl.tolist()) == {0, 1} and set(f12.tolist()) == {0, 1}, tag


# ---------------------------------------------------------------------------------------------------- inner product
@pytest.mark.parametrize("dim,n", [(65, 20000), (128, 20000), (960, 5000)])
def test_inner_product(gpu_pkg, dim, n):
    """s = -(q.v) ascending by (s, id) against the exact integer product, bit for bit; the zero query and the zero rows
    of nd_u8_ip_data give products of exactly zero, which come back as -0.0"""
    rng = np.random.default_rng(24000 + dim)
    base_u8, q_u8 = D.ip_data(rng, n, 48, dim)
    q = _f32(q_u8)
    ip = D.ip_int64(q_u8, base_u8)
    ref = D.topk_ref(ip, 16)
    assert not q_u8[D.ZERO_Q].any() and not base_u8[list(D.zero_rows(n))].any()
    with gpu_pkg.BruteForceIndex.from_u8(base_u8, metric=gpu_pkg.METRIC_IP) as idx:
        assert idx.getDim() == dim
        for k in (1, 5, 15):
            for call, nb, B in _shapes(dim):
                gi, gd, fl = _call(gpu_pkg, idx, q, nb, B, k, call)
                m = nb * B
                wi, wd = ref[0][:m, :k + 1], ref[1][:m, :k + 1]
                tag = (dim, k, call, nb, B)
                assert np.array_equal(bits(gd), bits(wd)), tag
                assert np.array_equal(gi, wi), tag
                assert np.array_equal(fl, D.tie_flags(wd)), tag
                if m > D.ZERO_Q:
                    assert (bits(gd[D.ZERO_Q]) == np.int32(-2 ** 31)).all(), "a zero product is -0.0"
                    assert np.array_equal(gi[D.ZERO_Q], np.arange(k + 1))


# ---------------------------------------------------------------------------------------------------- refused batches
def _refusal_data():
    """values under 16 (and the planted 0 / 255) at dim 200: ||q||^2 < 2^18, so that the fp32 reference stays exact with
    a query value of 0.5 as well (every partial sum is a multiple of 1/4 below 2^22)"""
    rng = np.random.default_rng(25000)
    base_u8, q_u8 = u8_data(rng, 20000, 48, 200, hi=16)
    assert 4 * (sqnorm_max(base_u8) + sqnorm_max(q_u8) + 256 ** 2) < 2 ** 24
    return base_u8, _f32(base_u8), _f32(q_u8)


def _assert_refused(got, tag):
    gi, gd, fl = got
    assert (fl == 2).all(), (tag, fl)
    assert (gi == -1).all() and np.isposinf(gd).all(), tag


@pytest.mark.parametrize("value", [0.5, -1.0, 256.0])
def test_a_value_that_is_no_byte_refuses_its_batch(gpu_pkg, value):
    base_u8, base, q = _refusal_data()
    k, B = 5, 16
    bad = q.copy()
    bad[B + 4, 10] = value  # batch 1 of a 3 x 16 call
    oi, od = oracle.search_bf(base, q, k + 1)
    sref = _sorted_int_ref(base, q, k + 2)
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
        for nq in (16, 7, 5):  # one batch through vs_bf_search_dev; the bad query is its fifth, at nq = 5 the last
            _assert_refused(_call(gpu_pkg, idx, bad[B:], 1, nq, k, "one"), (value, nq))
        s = slice(B, B + 4)  # ... and a batch that ends before it runs on the bytes
        _check_int(_call(gpu_pkg, idx, bad[B:], 1, 4, k, "one"), oi[s], od[s], (sref[0][s], sref[1][s]), (value, "4 queries"))
        gi, gd, fl = _call(gpu_pkg, idx, bad, 3, B, k, "multi")
        _assert_refused((gi[B:2 * B], gd[B:2 * B], fl[B:2 * B]), (value, "middle batch"))
        for b in (0, 2):
            s = slice(b * B, (b + 1) * B)
            _check_int((gi[s], gd[s], fl[s]), oi[s], od[s], (sref[0][s], sref[1][s]), (value, "batch", b))
        # the host call reruns the refused batch on the fp32 rows: the oracle's answer, ties resolved
        idx.set_batch(B)
        hi, hd = idx.search(bad, k)
    wi, wd = oracle.search_bf(base, bad, k)
    assert np.array_equal(hd, wd) and np.array_equal(hi, wi), value


def test_norm_rule_refuses_to_the_unit(gpu_pkg):
    """||q||^2 + max ||b||^2 <= 2^24 at dim 2048: a batch exactly on the bound runs on the bytes and is exact, one unit
    above it and far above it (a query of 255s) are refused"""
    rng = np.random.default_rng(25500)
    dim, n, B, k = 2048, 5000, 16, 5
    base_u8 = rng.integers(0, 41, size=(n, dim)).astype(np.uint8)
    bmax = sqnorm_max(base_u8)
    q_u8 = rng.integers(0, 41, size=(3 * B, dim)).astype(np.uint8)
    q_u8[7] = _with_sqnorm(2 ** 24 - bmax, dim)              # batch 0: on the bound
    q_u8[B + 5] = 255                                        # batch 1: far above it
    q_u8[2 * B + 9] = _with_sqnorm(2 ** 24 - bmax + 1, dim)  # batch 2: one above it
    # the precondition, on the CPU: the base keeps its byte copy, batch 0 passes the rule, batches 1 and 2 do not
    assert bmax < 2 ** 24
    assert sqnorm_max(q_u8[:B]) + bmax == 2 ** 24
    assert sqnorm_max(q_u8[B:2 * B]) + bmax > 2 ** 24 and sqnorm_max(q_u8[2 * B:]) + bmax == 2 ** 24 + 1
    base, q = _f32(base_u8), _f32(q_u8)
    oi, od = oracle.search_bf(base, q[:B], k + 1)
    sref = _sorted_int_ref(base, q[:B], k + 2)
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
        gi, gd, fl = _call(gpu_pkg, idx, q, 3, B, k, "multi")
        _check_int((gi[:B], gd[:B], fl[:B]), oi, od, sref, "on the bound")
        _assert_refused((gi[B:], gd[B:], fl[B:]), "above the bound")
        _assert_refused(_call(gpu_pkg, idx, q[2 * B:], 1, B, k, "one"), "one above the bound")
        got = idx.search(q, k)
        idx.set_precision(1)
        want = idx.search(q, k)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    hi, hd = oracle.search_bf(base, q[:B], k)
    assert np.array_equal(got[0][:B], hi) and np.array_equal(got[1][:B], hd)


# ---------------------------------------------------------------------------------------------------- properties of the route
def test_result_does_not_depend_on_the_route(gpu_pkg, tmp_path):
    """the same indexes in a child process under VSEARCH_ND_ONE_U8=0 (the per-batch byte scan): ids, distance bits and
    flags are equal, the refused batch included, and the child made no single-call launch on the byte rows.  Precision 1
    on the default index takes route 2."""
    out = str(tmp_path / "per_batch.npz")
    r = subprocess.run([sys.executable, os.path.abspath(nd_one_u8_child.__file__), ROOT, out],
                       env=dict(os.environ, VSEARCH_ND_ONE_U8="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ND_ONE_U8_CHILD_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1500:])
    child = np.load(out)
    assert os.environ.get("VSEARCH_ND_ONE_U8", "1") != "0"
    here = nd_one_u8_child.run(gpu_pkg)
    dims = {name: c[0].shape[1] for name, c in nd_one_u8_child.cases().items()}
    seen = set()
    for key in here:
        if key.endswith("_stats"):
            launches = sum(nb for _, nb, B in nd_one_u8_child.SHAPES if not _excepted(dims[key[:-6]], B)) * len(nd_one_u8_child.KS)
            assert launches >= 18
            assert tuple(child[key]) == (0, 0), key
            assert tuple(here[key]) == (0, launches), key
        elif key.endswith("_d"):
            assert np.array_equal(bits(here[key]), bits(child[key])), key
        else:
            assert np.array_equal(here[key], child[key]), key
            if key.endswith("_f"):
                seen |= set(here[key].tolist())
    assert seen == {0, 1, 2}
    f = here["l2_200_refused_5_multi_3_16_f"]
    assert (f[16:32] == 2).all() and not (f[:16] == 2).any() and not (f[32:] == 2).any()
    # precision 1: the fp32 rows, on scan_one_nd_kernel
    base_u8, q, _ = nd_one_u8_child.cases()["l2_320"]
    assert gpu_pkg.BruteForceIndex.one_plan(len(base_u8), 320, _cus(), 3, 16, 5)[0] == 2
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx:
        idx.set_precision(1)
        got = tc._bf_dev(idx, q, 3, 16, 5, "multi")
        assert idx.one_stats() == (3, 0)
        assert idx.one_stats(reset=True) == (3, 0) and idx.one_stats() == (0, 0)
    assert _same_bits(got, tuple(here[f"l2_320_5_multi_3_16_{x}"] for x in "idf"))


def test_neighbours_keep_their_routes(gpu_pkg):
    """B = 17, 4 batches and k = 16 on the same index make no single-call launch on the byte rows and match the oracle;
    id_offset is carried; calls interleaved with a second, fp32 general index in the same process still match (each
    launch leaves the arrival counter of its index at its start value)."""
    rng = np.random.default_rng(26000)
    n, dim, k = 20000, 200, 5
    base_u8, q_u8 = u8_data(rng, n, 64, dim)
    base, q = _f32(base_u8), _f32(q_u8)
    plan = gpu_pkg.BruteForceIndex.one_plan_u8
    assert plan(n, dim, _cus(), 1, 17, k)[0] == 0 and plan(n, dim, _cus(), 4, 16, k)[0] == 0 and plan(n, dim, _cus(), 1, 16, 16)[0] == 0
    oi, od = oracle.search_bf(base, q, k + 1)
    sref = _sorted_int_ref(base, q, 18)
    with gpu_pkg.BruteForceIndex.from_u8(base_u8) as idx, gpu_pkg.BruteForceIndex(base[:6000]) as other:
        _check_int(_call(gpu_pkg, idx, q, 1, 17, k, "one", byte_launches=0), oi[:17], od[:17], sref, "B = 17")
        _check_int(_call(gpu_pkg, idx, q, 4, 16, k, "multi", byte_launches=0), oi, od, sref, "4 batches")
        gi, gd, fl = _call(gpu_pkg, idx, q, 1, 16, 16, "topk", byte_launches=0)
        assert np.array_equal(gd, sref[1][:16, :17]) and set(np.unique(fl)) <= {0, 1}
        assert np.array_equal(gi[fl == 0][:, :16], sref[0][:16][fl == 0][:, :16])
        assert idx.one_stats() == (0, 0)
        # interleaved with an fp32 general index (route 2 there)
        o_oi, o_od = oracle.search_bf(base[:6000], q, k + 1)
        o_sref = _sorted_int_ref(base[:6000], q, k + 2)
        for rep in range(3):
            _check_int(_call(gpu_pkg, idx, q, 3, 16, k, "multi"), oi[:48], od[:48], sref, ("byte", rep))
            _check_int(tc._bf_dev(other, q, 3, 16, k, "multi"), o_oi[:48], o_od[:48], o_sref, ("fp32", rep))
            _check_int(_call(gpu_pkg, idx, q, 1, 7, k, "one"), oi[:7], od[:7], sref, ("byte one", rep))
        assert idx.one_stats() == (0, 12) and other.one_stats() == (9, 0)
    wi, wd = _sorted_int_ref(base[:5000], q[:16], k + 1, id_offset=1000)
    with gpu_pkg.BruteForceIndex.from_u8(base_u8[:5000], id_offset=1000) as idx:
        gi, gd, fl = _call(gpu_pkg, idx, q, 1, 16, k, "one")
    assert np.array_equal(gd, wd) and np.array_equal(gi, wi) and gi.min() >= 1000


def test_stats_refuse_a_null_output_and_an_ivf_index(gpu_pkg):
    import ctypes as C
    out = (C.c_int64 * 2)(-9, -9)
    base = gpu_pkg.synth_sift(2000, seed=5)
    with gpu_pkg.BruteForceIndex(base) as bf:
        assert gpu_pkg.lib().vs_bf_one_stats(bf._h, None, 0) == -1
        assert gpu_pkg.lib().vs_bf_one_stats(bf._h, out, 0) == 0 and list(out) == [0, 0]
    vr, off, r2o = gpu_pkg.ivf_layout_from_assignment(base, np.arange(2000) % 8, 8)
    with _open_ivf(gpu_pkg, vr, base[:8].copy(), off, r2o) as ivf:
        assert gpu_pkg.lib().vs_bf_one_stats(ivf._h, out, 0) == -1
