"""Host-side checks of the cross-list merge's ABI (vs_topk_merge_dev, vs_topk_merge_plan): symbols, the kernel choice at
its boundaries, every refused argument (all refused before any device work), and the numpy reference of
tests/merge_ref.py on cases whose answers are written out here.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merge_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in ("vs_topk_merge_dev", "vs_topk_merge_plan"):
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)
    assert hasattr(pkg, "topk_merge_dev") and hasattr(pkg, "topk_merge_plan")


@pytest.mark.parametrize("G,kin,lpt", [
    (64, 64, 0), (1, 4096, 0), (4096, 1, 0), (16384, 1, 64), (20000, 1, None),  # (the cap counts entries, not lists)
    (1, 4097, 1), (4097, 1, 32), (241, 17, 1),                                       # 4097 entries: the first past the cap
    (256, 17, 1), (257, 17, 2), (512, 17, 2), (513, 17, 4), (1024, 17, 4), (1025, 17, 8), (2048, 17, 8), (2049, 17, 16),
    (4096, 17, 16), (4097, 17, 32), (8192, 17, 32), (8193, 17, 64), (16384, 17, 64), (16385, 17, None), (16385, 1, None),
])
def test_plan_at_the_boundaries(pkg, G, kin, lpt):
    out = (C.c_int64 * 3)(7, 7, 7)
    rc = pkg.lib().vs_topk_merge_plan(G, kin, 10, out)
    if lpt is None:
        assert rc == -5 and list(out) == [7, 7, 7]
        assert b"16384" in pkg.lib().vs_last_error()
        with pytest.raises(pkg.VSearchError) as e:
            pkg.topk_merge_plan(G, kin, 10)
        assert e.value.status == -5
        return
    assert rc == 0 and list(out) == [lpt, 4096, 256]
    assert pkg.topk_merge_plan(G, kin, 10) == (lpt, ref.CAP, ref.TRACK)
    assert ref.head_lpt(G, kin) == lpt
    assert pkg.topk_merge_plan(G, kin, 1) == pkg.topk_merge_plan(G, kin, 100000)  # kout does not choose the kernel


def test_plan_is_4096_entries_exactly(pkg):
    for G in range(1, 70):
        kin = 4096 // G
        assert pkg.topk_merge_plan(G, kin, 5)[0] == 0
        assert pkg.topk_merge_plan(G, kin + 1, 5)[0] == 1  # G * (kin + 1) > 4096, G <= 256


@pytest.mark.parametrize("G,kin,kout", [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -3, 4), (4, 4, -2)])
def test_plan_refuses_counts_below_one(pkg, G, kin, kout):
    out = (C.c_int64 * 3)(7, 7, 7)
    assert pkg.lib().vs_topk_merge_plan(G, kin, kout, out) == -1
    assert list(out) == [7, 7, 7]
    assert pkg.lib().vs_topk_merge_plan(4, 4, 4, None) == -1


def test_merge_refuses_before_any_device_work(pkg):
    """Dummy non-null pointers: every call here must return from the argument checks (none of them may reach a launch)."""
    L = pkg.lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)

    def call(d=p, i=p, G=4, B=3, kin=5, stride=0, kout=5, od=p, oi=p, fl=p):
        return L.vs_topk_merge_dev(d, i, G, B, kin, stride, kout, od, oi, fl, None)

    assert call(d=None) == -1 and call(i=None) == -1 and call(od=None) == -1 and call(oi=None) == -1
    assert call(G=0) == -1 and call(B=0) == -1 and call(kin=0) == -1 and call(kout=0) == -1 and call(G=-4) == -1
    # a stride below the dense one would alias the groups
    assert call(stride=-1) == -1
    assert b"stride_g" in L.vs_last_error() and b"15" in L.vs_last_error()
    assert call(stride=1) == -1 and call(stride=14) == -1
    assert call(stride=-(2 ** 40)) == -1
    # more lists than the list-head kernel takes: unsupported, not a device error
    assert call(G=16385, kin=1) == -5
    assert b"16384" in L.vs_last_error() and b"4096" in L.vs_last_error()
    assert call(G=16385, kin=1, fl=None) == -5 and call(G=2 ** 20, kin=7) == -5
    assert call(G=16385, kin=1, stride=5) == -5  # (a valid stride: 3 queries of one entry)
    # the null and count checks come first, whatever else is wrong
    assert call(d=None, G=16385, kin=1) == -1 and call(kout=0, stride=-1) == -1


# ------------------------------------------------------------------------------------------------ the reference itself
def _lists(rows):
    """rows[g] = [(dist, id), ...] of one query -> d, i [G, 1, kin]"""
    d = np.array([[[e[0] for e in r]] for r in rows], dtype=np.float32)
    i = np.array([[[e[1] for e in r]] for r in rows], dtype=np.int32)
    return d, i


def test_reference_tie_by_id_across_lists():
    d, i = _lists([[(-2.0, 9), (0.0, 7), (5.0, 1)],
                   [(-2.0, 4), (-0.0, 3), (INF, -1)],
                   [(-np.inf, ref.ID_MAX), (0.0, 5), (5.0, 0)]])
    od, oi, fl, M = ref.merge_ref(d, i, 8)
    assert M.tolist() == [8]
    assert oi.tolist() == [[ref.ID_MAX, 4, 9, 3, 5, 7, 0, 1]]
    # the zero of id 3 keeps its sign bit
    assert ref.bits(od).tolist() == [ref.bits(np.array([-np.inf, -2, -2, -0.0, 0.0, 0.0, 5, 5], dtype=np.float32)).tolist()]
    assert fl.tolist() == [1]
    od, oi, fl, _ = ref.merge_ref(d, i, 2)  # (-inf, -2): no two equal among the first two
    assert oi.tolist() == [[ref.ID_MAX, 4]] and fl.tolist() == [0]


def test_reference_list_ended_by_nan_and_the_other_ends():
    d, i = _lists([[(1.0, 10), (NAN, 11), (-5.0, 12), (-4.0, 13)],     # NaN ends it: -5 and -4 are never seen
                   [(2.0, 20), (INF, 21), (-6.0, 22), (-3.0, 23)],     # +inf with an id ends it
                   [(3.0, 30), (-7.0, -1), (-6.5, 32), (-2.0, 33)],    # a negative id ends it
                   [(NAN, 40), (0.0, 41), (0.5, 42), (0.75, 43)],      # empty
                   [(4.0, 50), (4.0, 51), (4.5, 52), (6.0, 53)]])      # full
    assert ref.list_lengths(d, i)[:, 0].tolist() == [1, 1, 1, 0, 4]
    od, oi, fl, M = ref.merge_ref(d, i, 7)
    assert M.tolist() == [7]
    assert oi.tolist() == [[10, 20, 30, 50, 51, 52, 53]]
    assert od.tolist() == [[1.0, 2.0, 3.0, 4.0, 4.0, 4.5, 6.0]]
    assert fl.tolist() == [1]
    assert ref.merge_ref(d, i, 4)[2].tolist() == [0]  # 1, 2, 3, 4: the second 4 is output 5


def test_reference_kout_past_the_pool():
    d, i = _lists([[(0.5, 2), (INF, -1)], [(INF, -1), (INF, -1)], [(0.25, 8), (0.5, 1)]])
    od, oi, fl, M = ref.merge_ref(d, i, 6)
    assert M.tolist() == [3]
    assert oi.tolist() == [[8, 1, 2, -1, -1, -1]]
    assert od.tolist() == [[0.25, 0.5, 0.5, np.inf, np.inf, np.inf]]
    assert fl.tolist() == [1]  # 0.5 twice; the +inf tail is no tie
    d, i = _lists([[(INF, -1)], [(NAN, 3)]])
    od, oi, fl, M = ref.merge_ref(d, i, 3)
    assert M.tolist() == [0] and oi.tolist() == [[-1, -1, -1]] and np.all(od == INF) and fl.tolist() == [0]


def test_reference_flag_window_is_256_outputs():
    d = np.arange(300, dtype=np.float32).reshape(1, 1, 300).copy()
    i = np.arange(300, dtype=np.int32).reshape(1, 1, 300).copy()
    d[0, 0, 271] = d[0, 0, 270]
    assert ref.merge_ref(d, i, 300)[2].tolist() == [0]
    d[0, 0, 256] = d[0, 0, 255]  # outputs 255 / 256: the second is outside the window
    assert ref.merge_ref(d, i, 300)[2].tolist() == [0]
    d[0, 0, 255] = d[0, 0, 254]
    assert ref.merge_ref(d, i, 300)[2].tolist() == [1]


def test_generator_keeps_the_contract_and_mixes_what_it_should():
    d, i = ref.generate(3, 64, 64, [0, 1, 64, 600, 4096])
    lens = ref.list_lengths(d, i)
    assert lens.sum(0).tolist() == [0, 1, 64, 600, 4096]
    seen = set()
    for b in range(d.shape[1]):
        pool = []
        for g in range(64):
            L = lens[g, b]
            dd, ii = d[g, b, :L], i[g, b, :L]
            assert np.all(dd < INF) and np.all(ii >= 0) and np.all(ii <= ref.ID_MAX)
            assert np.array_equal(np.lexsort((ii, dd)), np.arange(L))  # ascending by (dist, id)
            pool += ii.tolist()
            if L < 64:
                e = d[g, b, L]
                seen.add("nan" if e != e else "inf" if i[g, b, L] >= 0 else "neg" if e < INF else "pad")
        assert len(set(pool)) == len(pool)  # distinct across the query's lists
        assert not pool or ref.ID_MAX in pool
    assert seen == {"nan", "inf", "neg", "pad"}
    b600 = ref.bits(d[:, 3, :][np.arange(64)[None, :] < lens[:, 3, None]])
    for v in (-np.inf, -0.0, 0.0, ref.SUBNORMAL, -3.5):
        assert ref.bits(np.float32(v)) in b600
    assert ref.merge_ref(d, i, 16)[2].tolist() == [0, 0, 1, 1, 1]  # equal distances across lists


def test_routes_follow_the_kernel_source():
    assert [ref.compact_route(M, 128) for M in (0, 64, 65, 256, 257, 1024, 1025, 4096)] == \
        ["epl1", "epl1", "epl4", "epl4", "epl16", "epl16", "rounds", "rounds"]
    assert ref.compact_route(256, 64) == "epl4" and ref.compact_route(257, 64) == "filter" and ref.compact_route(257, 65) == "epl16"
    assert [ref.compact_route(2000, 64, S) for S in (64, 65, 256, 257, 512, 513)] == \
        ["filter-epl1", "filter-epl4", "filter-epl4", "filter-epl16", "filter-epl16", "overflow-rounds"]
    assert ref.compact_route(1024, 64, 513) == "overflow-epl16"
    # the append order of one wave: step j takes entry j of every list that has one, lists ascending
    d, i = _lists([[(1.0, 1), (2.0, 2), (INF, -1)], [(INF, -1)] * 3, [(0.5, 3), (0.75, 4), (9.0, 5)]])
    cd, ci = ref.append_order(d[:, 0, :], i[:, 0, :])
    assert ci.tolist() == [1, 3, 2, 4, 5] and cd.tolist() == [1.0, 0.5, 2.0, 0.75, 9.0]
