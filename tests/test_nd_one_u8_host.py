"""Host-side checks of the single-call byte scan's plan and counters (vs_bf_one_plan_u8, vs_bf_one_stats):
the symbols, the refusals in vs_bf_one_plan's order, route 3 exactly inside the rule and 0 just outside each edge, and the
geometry.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5
CUS = 256
ROW_LIMIT = 2 ** 31 - 1 - 128


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name, nargs in (("vs_bf_one_plan_u8", 7), ("vs_bf_one_stats", 3)):
        assert name in declared
        assert name in pkg.exported_symbols()
        fn = getattr(pkg.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int32
    assert callable(pkg.BruteForceIndex.one_plan_u8) and callable(pkg.BruteForceIndex.one_stats)


def _rc(pkg, n_rows, dim, cus, nb, B, k, out=True, fn="vs_bf_one_plan_u8"):
    buf = (C.c_int64 * 4)(-9, -9, -9, -9)
    return getattr(pkg.lib(), fn)(n_rows, dim, cus, nb, B, k, buf if out else None), list(buf)


def test_refusals_in_order(pkg):
    ok = (20000, 384, CUS, 1, 1, 5)
    assert _rc(pkg, *ok)[0] == 0
    assert _rc(pkg, *ok, out=False)[0] == INVALID
    for bad in ((0, 384, CUS, 1, 1, 5), (20000, 384, 0, 1, 1, 5), (20000, 384, CUS, 0, 1, 5), (20000, 384, CUS, 1, 0, 5),
                (20000, 384, CUS, 1, 33, 5), (20000, 384, CUS, 1, 1, 0)):
        rc, buf = _rc(pkg, *bad)
        assert rc == INVALID and buf == [-9] * 4, bad  # nothing is written on a refusal
    assert _rc(pkg, 20000, 0, CUS, 1, 1, 5)[0] == INVALID
    assert _rc(pkg, 20000, 2049, CUS, 1, 1, 5)[0] == UNSUPPORTED
    assert _rc(pkg, 20000, 384, CUS, 1, 1, 129)[0] == UNSUPPORTED
    assert _rc(pkg, 20000, 384, CUS, 1, 1, 128)[0] == 0
    # the order: the argument checks come before the dimension, dim < 1 before dim > 2048, the dimension before k > 128
    assert _rc(pkg, 0, 4096, CUS, 1, 1, 500)[0] == INVALID
    assert _rc(pkg, 20000, 0, CUS, 1, 1, 500)[0] == INVALID
    assert _rc(pkg, 20000, 4096, CUS, 1, 1, 500)[0] == UNSUPPORTED
    with pytest.raises(pkg.VSearchError) as e:
        pkg.BruteForceIndex.one_plan_u8(20000, 2049, CUS, 1, 1, 5)
    assert e.value.status == UNSUPPORTED and "2048" in str(e.value)
    # the same checks with the same codes as vs_bf_one_plan, case by case
    for args in (ok, (0, 384, CUS, 1, 1, 5), (20000, 384, CUS, 1, 33, 5), (20000, 0, CUS, 1, 1, 5), (20000, 2049, CUS, 1, 1, 5),
                 (20000, 384, CUS, 1, 1, 129), (0, 4096, CUS, 1, 1, 500), (20000, 4096, CUS, 1, 1, 500)):
        assert _rc(pkg, *args)[0] == _rc(pkg, *args, fn="vs_bf_one_plan")[0], args


def test_route_3_inside_the_rule_and_0_outside_each_edge(pkg):
    """fewer than 4 batches, B <= 16, k <= 15, n_rows <= 2^31 - 1 - 128 -- and the measured exception: rows
    of at most 128 bytes (dim <= 128) keep the per-batch route for more than 12 queries"""
    plan = pkg.BruteForceIndex.one_plan_u8
    for dim in (1, 64, 128, 129, 192, 2048):  # (the byte form of a 128-d index is general under inner product)
        top = 12 if dim <= 128 else 16  # the most queries of a batch on route 3
        for nb in (1, 2, 3):
            for B in (1, 7, top):
                for k in (1, 5, 15):
                    assert plan(20000, dim, CUS, nb, B, k)[0] == 3, (dim, nb, B, k)
        assert plan(20000, dim, CUS, 3, top, 15)[0] == 3
        assert plan(20000, dim, CUS, 4, top, 15) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 3, top + 1, 15) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 3, 17, 15) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 3, top, 16) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 1, 32, 128) == (0, 0, 0, 0)
        assert plan(ROW_LIMIT, dim, CUS, 3, top, 15)[0] == 3
        assert plan(ROW_LIMIT + 1, dim, CUS, 3, top, 15) == (0, 0, 0, 0)
        assert (plan(20000, dim, CUS, 1, 16, 5)[0] == 3) == (dim > 128)
        assert (plan(20000, dim, CUS, 1, 13, 5)[0] == 3) == (dim > 128)


def test_geometry(pkg):
    plan = pkg.BruteForceIndex.one_plan_u8
    assert plan(1, 100, CUS, 1, 1, 5) == (3, 1, 64, 1)
    assert plan(64, 100, CUS, 1, 1, 5) == (3, 1, 64, 1)
    assert plan(65, 100, CUS, 1, 1, 5) == (3, 1, 64, 1)       # two units: two waves of one workgroup
    assert plan(8 * 64 + 1, 100, CUS, 1, 1, 5) == (3, 2, 64, 1)
    for cus in (1, 8, 64, 256, 1000):
        for n in (1, 63, 64, 65, 512, 513, 4099, 20000, 10 ** 6, ROW_LIMIT):
            route, grid, unit, most = plan(n, 200, cus, 1, 16, 15)
            units = -(-n // 64)
            assert (route, unit) == (3, 64)
            assert grid == min(cus, 256, -(-units // 8)), (cus, n)
            assert most == -(-units // (grid * 8)), (cus, n)
        # a multiple of a full run (grid x 8 waves x 64 rows), one row less and one more
        grid = min(cus, 256)
        run = grid * 8 * 64
        assert plan(3 * run - 1, 200, cus, 1, 16, 15) == (3, grid, 64, 3)
        assert plan(3 * run, 200, cus, 1, 16, 15) == (3, grid, 64, 3)
        assert plan(3 * run + 1, 200, cus, 1, 16, 15) == (3, grid, 64, 4)
    # the dimension does not enter the geometry, and it is route 2's
    assert plan(400000, 1, CUS, 1, 1, 5)[1:] == plan(400000, 2048, CUS, 1, 1, 5)[1:] == plan(400000, 20, CUS, 3, 12, 15)[1:]
    assert plan(400000, 300, CUS, 1, 1, 5)[1:] == pkg.BruteForceIndex.one_plan(400000, 300, CUS, 1, 1, 5)[1:]


def test_stats_without_an_index_are_refused(pkg):
    out = (C.c_int64 * 2)(-9, -9)
    assert pkg.lib().vs_bf_one_stats(None, out, 0) == INVALID  # refused before any device is touched
    assert list(out) == [-9, -9]
    assert b"vs_bf_one_stats" in pkg.lib().vs_last_error()
