"""Host-side checks of the single-call half-row scan's plan and counter (vs_bf_one_plan_f16, vs_bf_one_f16_stats, DESIGN
4.4i): refusals in vs_bf_one_plan's order, route 4 inside the rule and 0 outside each edge, route 2's geometry.  No GPU."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -5
CUS = 256
ROW_LIMIT = 2 ** 31 - 1 - 128


def _rc(pkg, args, fn="vs_bf_one_plan_f16", out=True):
    buf = (C.c_int64 * 4)(-9, -9, -9, -9)
    return getattr(pkg.lib(), fn)(*args, buf if out else None), list(buf)


def test_refusals_in_order(pkg):
    ok = (20000, 384, CUS, 1, 1, 5)
    cases = [ok, (0, 384, CUS, 1, 1, 5), (20000, 384, 0, 1, 1, 5), (20000, 384, CUS, 0, 1, 5), (20000, 384, CUS, 1, 0, 5),
             (20000, 384, CUS, 1, 33, 5), (20000, 384, CUS, 1, 1, 0), (20000, 0, CUS, 1, 1, 5), (20000, 2049, CUS, 1, 1, 5),
             (20000, 384, CUS, 1, 1, 129), (20000, 384, CUS, 1, 1, 128),
             # the order: the argument checks before the dimension, dim < 1 before dim > 2048, the dimension before k > 128
             (0, 4096, CUS, 1, 1, 500), (20000, 0, CUS, 1, 1, 500), (20000, 4096, CUS, 1, 1, 500)]
    want = [0] + [INVALID] * 7 + [UNSUPPORTED, UNSUPPORTED, 0, INVALID, INVALID, UNSUPPORTED]
    for args, code in zip(cases, want):
        rc, buf = _rc(pkg, args)
        assert rc == code and (rc == 0 or buf == [-9] * 4), args  # nothing is written on a refusal
        assert rc == _rc(pkg, args, fn="vs_bf_one_plan")[0], args
    assert _rc(pkg, ok, out=False)[0] == INVALID


@pytest.mark.parametrize("dim", [1, 96, 128, 2048])
def test_route_4_inside_the_rule_and_0_outside_each_edge(pkg, dim):
    """fewer than 4 batches, B <= 16, k <= 15, n_rows <= 2^31 - 1 - 128; no measured exception"""
    plan = pkg.BruteForceIndex.one_plan_f16
    for nb, B, k in ((1, 1, 1), (2, 7, 5), (3, 16, 15)):
        assert plan(20000, dim, CUS, nb, B, k)[0] == 4, (dim, nb, B, k)
    for nb, B, k in ((4, 16, 15), (3, 17, 15), (3, 16, 16)):
        assert plan(20000, dim, CUS, nb, B, k) == (0, 0, 0, 0), (dim, nb, B, k)
    assert plan(ROW_LIMIT, dim, CUS, 3, 16, 15)[0] == 4 and plan(ROW_LIMIT + 1, dim, CUS, 3, 16, 15) == (0, 0, 0, 0)


def test_geometry_is_route_2s(pkg):
    for cus in (1, 8, 256, 1000):
        for n in (1, 63, 64, 65, 513, 4099, 10 ** 6, ROW_LIMIT):
            got = pkg.BruteForceIndex.one_plan_f16(n, 200, cus, 1, 16, 15)
            assert got == (4,) + pkg.BruteForceIndex.one_plan(n, 200, cus, 1, 16, 15)[1:] and got[2] == 64, (cus, n)


def test_stats_without_an_index_are_refused(pkg):
    out = (C.c_int64 * 1)(-9)
    assert pkg.lib().vs_bf_one_f16_stats(None, out, 0) == INVALID  # refused before any device is touched
    assert list(out) == [-9] and b"vs_bf_one_f16_stats" in pkg.lib().vs_last_error()
