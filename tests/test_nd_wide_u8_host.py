"""Host-side checks of the wide-k byte route's plan and counters (vs_bf_wide_plan, vs_bf_wide_stats): the
symbols, the refusals in their order, the prefix formula at its edges, and the null handle.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5
CAP = 8192


def prefix(n, k):
    """min(n, roundup4096(max(512 (k + 1), n (k + 1) / 2048)))"""
    l = max(512 * (k + 1), n * (k + 1) // 2048)
    return min(n, (l + 4095) // 4096 * 4096)


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name, nargs in (("vs_bf_wide_plan", 4), ("vs_bf_wide_stats", 3)):
        assert name in declared
        assert name in pkg.exported_symbols()
        fn = getattr(pkg.lib(), name)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int32
    assert callable(pkg.BruteForceIndex.wide_plan) and callable(pkg.BruteForceIndex.wide_stats)


def _rc(pkg, n_rows, dim, k, out=True):
    buf = (C.c_int64 * 3)(-9, -9, -9)
    return pkg.lib().vs_bf_wide_plan(n_rows, dim, k, buf if out else None), list(buf)


def test_refusals_in_order(pkg):
    ok = (20000, 384, 100)
    assert _rc(pkg, *ok)[0] == 0
    assert _rc(pkg, *ok, out=False)[0] == INVALID
    for bad in ((0, 384, 100), (-5, 384, 100), (20000, 384, 0), (20000, 384, -1)):
        rc, buf = _rc(pkg, *bad)
        assert rc == INVALID and buf == [-9] * 3, bad  # nothing is written on a refusal
    assert _rc(pkg, 20000, 0, 100) == (INVALID, [-9] * 3)
    assert _rc(pkg, 20000, 2049, 100) == (UNSUPPORTED, [-9] * 3)
    assert _rc(pkg, 20000, 384, 129) == (UNSUPPORTED, [-9] * 3)
    assert _rc(pkg, 20000, 2048, 128)[0] == 0
    # the order: the argument checks come before the dimension, dim < 1 before dim > 2048, the dimension before k > 128
    assert _rc(pkg, 0, 4096, 500)[0] == INVALID
    assert _rc(pkg, 20000, 4096, 0)[0] == INVALID
    assert _rc(pkg, 20000, 0, 500)[0] == INVALID
    assert _rc(pkg, 20000, 4096, 500)[0] == UNSUPPORTED
    pkg.lib().vs_bf_wide_plan(20000, 384, 129, (C.c_int64 * 3)())
    assert b"vs_bf_wide_plan" in pkg.lib().vs_last_error()
    with pytest.raises(pkg.VSearchError) as e:
        pkg.BruteForceIndex.wide_plan(20000, 2049, 100)
    assert e.value.status == UNSUPPORTED and "2048" in str(e.value)


def test_prefix_formula_at_its_edges(pkg):
    plan = pkg.BruteForceIndex.wide_plan
    # the sizes the GPU tests lean on
    assert [plan(10 ** 5, 96, k)[1] for k in (16, 50, 100, 128)] == [12288, 28672, 53248, 69632]
    for dim in (1, 96, 128, 2048):
        for k in (16, 17, 50, 100, 128):
            p0 = (512 * (k + 1) + 4095) // 4096 * 4096  # the shortest prefix of this k
            for n in (1, 20, k, k + 1, 4095, 4096, 4097, p0 - 1, p0, p0 + 1, p0 + 209, 2 * p0, 10 ** 6, 10 ** 7, 2 ** 31 - 1):
                assert plan(n, dim, k) == (1, prefix(n, k), CAP), (n, dim, k)
            assert plan(p0 - 1, dim, k)[1] == p0 - 1 and plan(p0, dim, k)[1] == p0 and plan(p0 + 1, dim, k)[1] == p0
        # where the prefix starts to grow with the base: n (k + 1) / 2048 passes a multiple of 4096
        k = 128
        n = -(-(69632 + 1) * 2048 // 129)  # the first n with n (k + 1) / 2048 > 69632, the shortest prefix of k = 128
        for m in (n - 2, n - 1, n, n + 1):
            assert plan(m, dim, k)[1] == prefix(m, k)
        assert plan(n, dim, k)[1] == 69632 + 4096 and plan(n - 1, dim, k)[1] == 69632
        # k <= 15 is not a wide call: all three are zero
        for k in (1, 5, 15):
            assert plan(10 ** 6, dim, k) == (0, 0, 0)
        assert plan(10 ** 6, dim, 16)[0] == 1 and plan(1, dim, 128) == (1, 1, CAP)


def test_stats_without_an_index_are_refused(pkg):
    out = (C.c_int64 * 3)(-9, -9, -9)
    assert pkg.lib().vs_bf_wide_stats(None, out, 0) == INVALID  # refused before any device is touched
    assert list(out) == [-9, -9, -9]
    assert b"vs_bf_wide_stats" in pkg.lib().vs_last_error()
