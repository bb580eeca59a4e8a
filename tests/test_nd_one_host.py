"""Host-side checks of the single-call scan's plan (vs_bf_one_plan, BruteForceIndex.one_plan): the symbol, the refusals in
their order, which kernel a call shape takes, and the geometry of the general-dimension kernel.  No GPU needed."""
import ctypes as C
import os

import pytest

INVALID, UNSUPPORTED = -1, -5
CUS = 256


def test_symbol_and_binding(pkg):
    assert hasattr(pkg.lib(), "vs_bf_one_plan")
    assert callable(pkg.BruteForceIndex.one_plan)
    with open(os.path.join(os.path.dirname(pkg.LIB_PATH), "..", "include", "vsearch.h")) as f:
        assert "vs_bf_one_plan" in f.read()


def _rc(pkg, n_rows, dim, cus, nb, B, k, out=True):
    buf = (C.c_int64 * 4)(-9, -9, -9, -9)
    return pkg.lib().vs_bf_one_plan(n_rows, dim, cus, nb, B, k, buf if out else None), list(buf)


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
        pkg.BruteForceIndex.one_plan(20000, 2049, CUS, 1, 1, 5)
    assert e.value.status == UNSUPPORTED and "2048" in str(e.value)


def test_routes(pkg):
    plan = pkg.BruteForceIndex.one_plan
    assert os.environ.get("VSEARCH_ND_FORCE", "0") == "0"  # (it would make the general index the one at dim 128 too)
    assert plan(20000, 128, CUS, 1, 1, 5)[0] == 1
    for dim in (1, 127, 129, 2048):
        for nb, B, k in ((1, 1, 5), (3, 16, 15), (1, 7, 1)):
            assert plan(20000, dim, CUS, nb, B, k)[0] == 2, (dim, nb, B, k)
    for dim in (128, 384):
        assert plan(20000, dim, CUS, 3, 16, 15)[0] != 0
        assert plan(20000, dim, CUS, 4, 16, 15) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 3, 17, 15) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 3, 16, 16) == (0, 0, 0, 0)
        assert plan(20000, dim, CUS, 1, 32, 128) == (0, 0, 0, 0)


def test_geometry_of_the_general_kernel(pkg):
    plan = pkg.BruteForceIndex.one_plan
    assert plan(1, 100, CUS, 1, 1, 5) == (2, 1, 64, 1)
    assert plan(64, 100, CUS, 1, 1, 5) == (2, 1, 64, 1)
    assert plan(65, 100, CUS, 1, 1, 5) == (2, 1, 64, 1)       # two units: two waves of one workgroup
    assert plan(8 * 64 + 1, 100, CUS, 1, 1, 5) == (2, 2, 64, 1)
    prev = (0, 0)
    for n in (1, 63, 64, 65, 512, 513, 4099, 20000, 131072, 131073, 400000, 1000000, 10 ** 7, 2 ** 31 - 200):
        route, grid, unit, most = plan(n, 20, CUS, 1, 16, 15)
        assert route == 2 and unit == 64 and 1 <= grid <= CUS
        units = -(-n // unit)
        assert grid * 8 * most >= units > grid * 8 * (most - 1)  # every unit has a wave, and some wave has `most`
        assert grid >= prev[0] and most >= prev[1], n           # monotone in n_rows
        prev = (grid, most)
    assert plan(1000000, 768, CUS, 1, 1, 5) == (2, 256, 64, 8)
    assert plan(1000000, 768, 64, 1, 1, 5) == (2, 64, 64, 31)
    assert plan(1000000, 768, 1000, 1, 1, 5)[1] == 256          # never more workgroups than partial-list slots
    # the dimension does not enter the geometry; the 128-d kernel has 16-row units
    assert plan(400000, 1, CUS, 1, 1, 5)[1:] == plan(400000, 2048, CUS, 1, 1, 5)[1:]
    assert plan(1000000, 128, CUS, 1, 1, 5) == (1, 256, 16, 31)
