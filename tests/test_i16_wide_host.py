"""Host-side checks of the int16 cosine runner's wide top-k (vs_i16_search_topk*, vs_i16_wide_plan, vs_i16_wide_stats):
symbols, null handles and the sampling rule of the header.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import i16_wide_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_i16_search_topk_dev", "vs_i16_search_topk", "vs_i16_wide_plan", "vs_i16_wide_stats")


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)
    for name in ("search_topk", "search_topk_dev", "wide_stats"):
        assert hasattr(pkg.I16Runner, name)
    assert hasattr(pkg, "i16_wide_plan")
    hpp = open(os.path.join(ROOT, "include", "vsearch.hpp")).read()
    assert "searchTopk" in hpp and "vs_i16_search_topk(" in hpp


def test_null_handle_and_null_pointers(pkg):
    L = pkg.lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    for k in (5, 100, 129):  # the handle is checked before k
        assert L.vs_i16_search_topk_dev(None, p, 1, 4, k, p, p, None) == -1
        assert L.vs_i16_search_topk(None, p, 4, k, p, p) == -1
    assert L.vs_i16_wide_stats(None, p, 0) == -1
    assert L.vs_i16_wide_plan(1000, 100, None) == -1


@pytest.mark.parametrize("k", [17, 100, 128])
@pytest.mark.parametrize("n_rows", [1, 64, 1088, 1089, 8192, 20483, 524325, 10 ** 6])
def test_plan_follows_the_stated_rule(pkg, n_rows, k):
    sg, stride, cap = pkg.i16_wide_plan(n_rows, k)
    assert (sg, stride, cap) == ref.plan_ref(n_rows, k)
    n_groups = (n_rows + 63) // 64
    assert cap == 8192 and 1 <= sg <= n_groups and stride >= 1 and (sg - 1) * stride < n_groups
    if sg < n_groups:  # the sample leaves out the last group, the only one that can be ragged, and holds 64 k rows
        assert (sg - 1) * stride <= n_groups - 2 and sg * 64 >= 64 * k
    else:
        assert stride == 1


def test_plan_known_values(pkg):
    assert pkg.i16_wide_plan(524325, 100) == (401, 20, 8192)  # ceil(524325 * 100 / 2048) = 25602 rows
    assert pkg.i16_wide_plan(1088, 17) == (17, 1, 8192)       # 64 k rows: the sample is the whole base
    assert pkg.i16_wide_plan(1089, 17) == (17, 1, 8192)       # 18 groups, the last one left out
    assert pkg.i16_wide_plan(20483, 128) == (128, 2, 8192)


@pytest.mark.parametrize("n_rows,k", [(1000, 16), (1000, 129), (1000, 0), (0, 100), (-5, 100)])
def test_plan_refuses(pkg, n_rows, k):
    out = (C.c_int64 * 3)(7, 7, 7)
    assert pkg.lib().vs_i16_wide_plan(n_rows, k, out) == -1
    assert list(out) == [7, 7, 7]
    with pytest.raises(pkg.VSearchError) as e:
        pkg.i16_wide_plan(n_rows, k)
    assert e.value.status == -1
