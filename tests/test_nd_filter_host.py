"""Host arithmetic of the bf16 prefilter of a general index: the error bound at any dimension, the hot test's
threshold, and vs_bf_filter_nd_plan's rule, refusals and geometry.  No GPU."""
import ctypes as C

import numpy as np
import pytest

ARGS = [(1e-3, 1.0, 1.0, 2.0, 4e-3, 2.0), (0.0, 0.0, 0.0, 1.0, 0.0, 1.0), (0.3, 511.0, 510.5, 498.0, 0.9, 497.5), (1e-9, 1e-6, 1e-6, 1e6, 1e3, 1e6)]


@pytest.mark.parametrize("a", ARGS)
def test_bound_at_128_and_growth_with_dim(pkg, a):
    L = pkg.lib()
    assert pkg.f32_filter_bound_nd(128, *a) == float(L.vs_f32_filter_bound(*a))
    e = [pkg.f32_filter_bound_nd(d, *a) for d in (1, 16, 17, 32, 33, 128, 400, 2048)]
    assert all(x <= y for x, y in zip(e, e[1:])) and e[0] > 0


def test_threshold_admits_what_the_exact_test_admits(pkg):
    """L2: a pair with d = RN(RN(qn + bn) - 2 S) < tau and |S - S'| <= E gives v = RN(2 S' - bn) > th; nothing is above +inf,
    everything above -inf."""
    fn = pkg.lib().vs_f32_filter_nd_th
    th = lambda metric, *v: fn(metric, *map(float, v))
    rng = np.random.default_rng(3)
    f = np.float32
    for _ in range(2000):
        qn, bn, nqp, bp = f(rng.uniform(0, 50)), f(rng.uniform(0, 50)), f(rng.uniform(0, 8)), rng.uniform(0, 8)
        e = f(rng.uniform(0, 1e-2))
        s = f(rng.uniform(-1, 1) * np.sqrt(qn * bn))
        d = f(np.float64(f(qn + bn)) - 2.0 * np.float64(s))
        tau = np.nextafter(d, f(np.inf))
        sp = f(np.float64(s) - np.float64(e))  # the worst bf16 sum the bound allows
        v = f(2.0 * np.float64(sp) - np.float64(bn))
        assert v > th(0, tau, qn, e, nqp, max(float(bn), 50.0), max(bp, float(np.sqrt(bn)))), (qn, bn, s, e)
        assert f(sp) > th(1, np.nextafter(f(-s), f(np.inf)), qn, e, nqp, 50.0, bp)
    inf = float("inf")
    assert th(0, inf, 1.0, 0.1, 1.0, 1.0, 1.0) == -inf and th(0, 1.0, 1.0, inf, 1.0, 1.0, 1.0) == -inf
    assert th(1, -inf, 1.0, 0.1, 1.0, 1.0, 1.0) == inf


def test_plan_refusals_in_order(pkg):
    L = pkg.lib()
    out = (C.c_int64 * 6)()
    cases = [((0, 0, 0, 0, 0), "at least 1"), ((1000, 0, 256, 4, 10), "dim must be at least 1"), ((1000, 4096, 256, 4, 10), "dim > 2048")]
    for args, msg in cases:
        assert L.vs_bf_filter_nd_plan(*args, out) != 0
        with pytest.raises(Exception, match=msg):
            pkg.bf_filter_nd_plan(*args)
    assert L.vs_bf_filter_nd_plan(1000, 64, 256, 4, 10, None) != 0


@pytest.mark.parametrize("n_rows", [1000000, 2000003, 3000000])
@pytest.mark.parametrize("nb", [4, 5, 9, 16, 17, 32])
def test_plan_geometry(pkg, n_rows, nb):
    """8 waves x column blocks per wave x passes cover the 2 nb column blocks with no empty pass; one wave buffer per wave
    (at most 256 workgroups in all); every workgroup owns a unit; the sample holds more than k + 1 distinct rows."""
    take, grid, passes, cbw, srows, stride = pkg.bf_filter_nd_plan(n_rows, 768, 256, nb, 10)
    assert take == 1 and 1 <= cbw <= 4 and passes == (1 if nb <= 16 else 2)
    assert 8 * cbw * passes >= 2 * nb > 8 * cbw * (passes - 1)
    assert 1 <= grid and grid * passes <= 256 and grid <= (n_rows + 63) // 64
    assert srows >= 256 and 1 <= stride <= 32 and (srows - 1) * stride < n_rows  # candidates per query do not grow with N


def test_plan_rule(pkg):
    assert pkg.bf_filter_nd_plan(1000000, 384, 256, 3, 10)[0] == 0    # short calls keep the single-call scan
    assert pkg.bf_filter_nd_plan(1000000, 384, 256, 33, 10)[0] == 0   # a launch group holds 32 batches
    assert pkg.bf_filter_nd_plan(1000000, 384, 256, 8, 16)[0] == 0    # wide k
    # measured shapes only: 96 <= dim <= 1024, 1 000 000 <= n_rows <= 3 000 000
    assert pkg.bf_filter_nd_plan(999999, 384, 256, 8, 10)[0] == 0 and pkg.bf_filter_nd_plan(3000001, 384, 256, 8, 10)[0] == 0
    assert pkg.bf_filter_nd_plan(1000000, 95, 256, 8, 10)[0] == 0 and pkg.bf_filter_nd_plan(1000000, 1025, 256, 8, 10)[0] == 0
    assert pkg.bf_filter_nd_plan(1000000, 96, 256, 8, 15)[0] == 1 and pkg.bf_filter_nd_plan(3000000, 1024, 256, 4, 1)[0] == 1


def test_symbols_exported(pkg):
    for name in ("vs_f32_filter_bound_nd", "vs_f32_filter_nd_th", "vs_bf_filter_nd_plan"):
        assert name in pkg.exported_symbols() and hasattr(pkg.lib(), name)
