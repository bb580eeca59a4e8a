"""Host-side checks of the per-call metric of the IVF search (vs_ivf_search_metric*): no GPU needed.  The data sets of
tests/test_gpu_ivf_nd_ip.py are checked here, against the oracle alone, for the edges they claim."""
import ctypes as C
import os
import re

import numpy as np

import ivf_ip_data as D
import near_ties
import oracle
from test_gpu_ivf_nd import EMPTY, NLIST

NAMES = ("vs_ivf_search_metric", "vs_ivf_search_metric_dev_multi")


def test_symbols_are_declared_and_exported(pkg):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)
    assert hasattr(pkg.IVFIndex, "search_metric") and hasattr(pkg.IVFIndex, "search_metric_dev_multi")


def test_null_arguments_come_first(pkg):
    L = pkg.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    # no index: VS_ERR_INVALID whatever the metric and k say
    assert L.vs_ivf_search_metric(None, p, 1, 129, 1, 7, p, p, None, None) == -1
    assert L.vs_ivf_search_metric_dev_multi(None, p, 1, 1, 0, 1, 7, p, p, None) == -1


def _neg_zero(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) == 0x80000000


def test_signed_set_empty_list_query():
    for dim in (1, 20):
        vr, cents, off, r2o, q = D.signed_index(dim)
        oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, 5, 1, return_probes=True, metric=1)
        assert probes[4, 0] == EMPTY and np.all(oi[4] == -1) and np.all(od[4] == np.inf)
        prod = q.astype(np.float64) @ vr.astype(np.float64).T
        assert (prod < 0).any() and (prod > 0).any()  # products of both signs


def test_negative_set_scores_and_best_lists():
    for dim in (20, 100):
        vr, cents, off, r2o, q = D.negative_index(dim)
        oi, od, _, probes = oracle.ivf_search(vr, off, r2o, cents, q, 16, 1, return_probes=True, metric=1)
        assert np.all(od > 0)  # (+inf in the empty slots included)
        assert probes[:4, 0].tolist() == [D.ONE_ROW, D.ROWS63, D.ROWS65, D.LAST], probes[:4, 0]
        assert oi[0, 0] == r2o[off[D.ONE_ROW]] and np.all(oi[0, 1:] == -1) and np.all(od[0, 1:] == np.inf)
        best4 = oracle.ivf_search(vr, off, r2o, cents, q, 5, 4, return_probes=True, metric=1)[3]
        for c in (D.ONE_ROW, D.ROWS63, D.ROWS65, D.LAST):
            assert (best4 == c).any()


def test_zeros_set_has_negative_zeros_between_the_signs():
    vr, cents, off, r2o, q, planted = D.zeros_index()
    for k in (5, 40):
        oi, od, _ = oracle.ivf_search(vr, off, r2o, cents, q, k, NLIST, metric=1)
        for i in D.ZERO_QUERIES:
            assert _neg_zero(od[i]).all()
            assert np.array_equal(oi[i], r2o[:k])  # equal scores: by position
    # an orthogonal query: negative scores (products > 0) first, then exact zeros, sign bit set, among them planted rows
    od = oracle.ivf_search(vr, off, r2o, cents, q, 4000, NLIST, metric=1)[1]
    for i in D.ORTH_QUERIES:
        z = _neg_zero(od[i])
        assert z.sum() >= len(planted) and (od[i] < 0).any() and (od[i][np.isfinite(od[i])] > 0).any()
        assert not (od[i].view(np.uint32) == 0).any()  # never +0.0


def test_duplicates_set_overflows_a_candidate_list():
    vr, cents, off, r2o, q = D.duplicates_index()
    oi, od, _ = oracle.ivf_search(vr, off, r2o, cents, q, 64, len(off) - 1, metric=1)
    assert np.array_equal(oi[2], r2o[300:364]) and np.all(od[2] == od[2][0])


def test_forced_coarse_near_ties_have_teeth():
    base, vr, cents, off, r2o, q, seeds = D.gauss_index(96)
    for nprobe in (1, 4):
        fq, mask = near_ties.boundary_queries(cents, seeds, nprobe, np.random.default_rng(77 + nprobe), metric=1)
        near_ties.require_teeth(mask, f"inner product, dim 96, nprobe {nprobe}")
