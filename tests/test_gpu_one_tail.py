"""The final merge of the two single-call scans (vs_one_tail.h) with 64 < M <= 256 candidates on DISTINCT distances.

The workgroup that arrives last reads the first entry of every workgroup's partial list, takes their k1-th smallest as the
bound, reads the lists whose first entry is not above it and ranks the M entries not above the bound: by counting for
M <= 64, by rounds from LDS for M <= 256, by rounds straight from the partial lists above that.  The all-zero
inner-product queries of test_gpu_ip.py and test_gpu_nd_one.py reach the two upper branches, but on all-equal distances
only (every flag set, every candidate at the bound).  Here M is 241 by construction and nothing ties:

    query 0, L2, k = 15 (k1 = 16), one query.  Row i = c_i e_1 with an integer c_i, so its distance is c_i^2, exact.
    Sixteen of the launch's 24 workgroups hold 16 planted rows each: in workgroups 0..14 the values 1..240 dealt round
    robin (workgroup w: w + 1, w + 16, ...), in workgroup 15 the values 241..256.  Every other row is 1000 or more.
    The partial lists' first entries are 1^2..15^2, 241^2 and eight above 1000^2: the bound is 241^2, sixteen lists pass,
    and of their 256 entries the 241 with c <= 241 are ranked.  The answer is the rows with c = 1..16, no flag.

Which rows a workgroup scans: the 128-d kernel deals 16-row tiles, tile t to workgroup t mod G; the general kernel deals
64-row units, 8 consecutive units to a workgroup (one run at these sizes).  G comes from BruteForceIndex.one_plan."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import oracle  # noqa: E402
import test_gpu_cancel as tc  # noqa: E402

pytestmark = pytest.mark.gpu

K = 15
G = 24


def _planted(n, dim, rows_of):
    """rows_of(w, j) = the row of workgroup w's j-th planted value"""
    c = 1000.0 + np.arange(n) % 3000  # (below 4096: c^2 is exact in fp32; equal values here are far above the bound)
    for w in range(15):
        for j in range(16):
            c[rows_of(w, j)] = w + 1 + 15 * j
    for j in range(16):
        c[rows_of(15, j)] = 241 + j
    assert np.array_equal(np.sort(c)[:256], np.arange(1, 257)) and np.sort(c)[256] >= 1000
    base = np.zeros((n, dim), dtype=np.float32)
    base[:, 0] = c
    return base, c


def _check(pkg, base, c, route):
    import torch
    n, dim = base.shape
    plan = pkg.BruteForceIndex.one_plan(n, dim, torch.cuda.get_device_properties(0).multi_processor_count, 1, 1, K)
    assert plan[:2] == (route, G), plan
    q = np.zeros((1, dim), dtype=np.float32)
    want_i = np.argsort(c, kind="stable")[:K + 1].astype(np.int32)[None, :]
    want_d = (c[want_i[0]] ** 2).astype(np.float32)[None, :]
    assert np.array_equal(c[want_i[0]], np.arange(1, K + 2))
    oi, od = oracle.search_bf(base, q, K + 1)
    assert np.array_equal(oi, want_i) and np.array_equal(od, want_d)
    with pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        for _ in range(2):  # (the walk over the rows alternates its direction)
            gi, gd, fl = tc._bf_dev(idx, q, 1, 1, K, "one")
            assert np.array_equal(gi, want_i), gi
            assert np.array_equal(gd, want_d), gd
            assert fl.tolist() == [0]


def test_128d_final_merge_by_rounds_from_lds(gpu_pkg):
    # 188 tiles; workgroup w has tiles w, w + 24, ..., w + 168: two planted rows in each of its eight
    base, c = _planted(3000, 128, lambda w, j: 16 * (w + G * (j % 8)) + j)
    _check(gpu_pkg, base, c, 1)


def test_general_final_merge_by_rounds_from_lds(gpu_pkg):
    # 192 units; workgroup w has units 8 w .. 8 w + 7 (rows 512 w .. 512 w + 511): two planted rows in each of its eight
    base, c = _planted(G * 512, 20, lambda w, j: 512 * w + 64 * (j % 8) + 3 * j)
    _check(gpu_pkg, base, c, 2)
