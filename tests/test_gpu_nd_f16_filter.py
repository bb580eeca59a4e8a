"""f16 MFMA prefilter of a float16 index: search_dev_multi under VSEARCH_ND_F16_FILTER=2 against the lists
ranked by (distance, id) from the chain oracle on the rows after rounding to float16 and widening -- ids, distance bits and
flags, no tolerance -- on gaussian rows, on self-queries over duplicated rows (distances cancel and tie) and on small
integers; many slabs, planted subnormals and values near the float16 range's end, inner product, overflow, and no route."""
import functools

import numpy as np
import pytest

import cancel_data
from test_gpu_nd_filter import _check, _dev, _ip_lists

pytestmark = pytest.mark.gpu

N = 4096 + 37  # the last 64-row unit is ragged
SHAPES = [(nb, B, k) for nb in (4, 9) for B in (32, 5) for k in (1, 15)]


@functools.lru_cache(maxsize=None)
def _data(kind, dim, nq=288):
    """(float16 base, fp32 queries, ids [nq, 16], distances [nq, 16]) made once and read-only"""
    rng = np.random.default_rng(1600 + dim)
    if kind == "gauss":
        base, q = rng.standard_normal((N, dim)).astype(np.float16), rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "cancel":  # the self-queries stay rows of the base, bit for bit, after the rounding
        b32, _, src = cancel_data.cancel_data(rng, N, nq, dim, 4)
        base = b32.astype(np.float16)
        q = base[src].astype(np.float32)
    elif kind == "same":
        base, q = np.tile(rng.standard_normal((1, dim)).astype(np.float16), (N, 1)), rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "ints":
        base, q = rng.integers(0, 9, size=(N, dim)).astype(np.float16), rng.integers(0, 9, size=(nq, dim)).astype(np.float32)
        base[N - 300:] = base[:300]
    else:  # "reals": test_gpu_nd_f16.py's recipe -- subnormals of both signs, a row of nothing else, values near +-6e4, duplicates
        base = rng.normal(0, 1, size=(N, dim)).astype(np.float16)
        sub = np.array([1, 2, 0x3FF, 0x8001, 0x83FF], dtype=np.uint16).view(np.float16)
        base[rng.integers(0, N, 400), rng.integers(0, dim, 400)] = sub[rng.integers(0, len(sub), 400)]
        base[5, :] = sub[np.arange(dim) % len(sub)]
        base[rng.integers(0, N, 6), rng.integers(0, dim, 6)] = np.float16(6.0e4) * np.array([1, -1, 1, -1, 1, -1], dtype=np.float16)
        base[N - 200:] = base[100:300]
        q = rng.normal(0, 1, size=(nq, dim)).astype(np.float32)
        q[:16] = base[[7, 100, 150, 299, 5, 64, 4098, 63] + list(range(2000, 2008))].astype(np.float32)
        q[20, 3] = 3.0e-6  # rounds to a float16 subnormal: written as zero in the sweep's operand
    ri, rd = cancel_data.sorted_scores(q, base.astype(np.float32), 16)
    for a in (base, q, ri, rd):
        a.setflags(write=False)
    return base, q, ri, rd


@pytest.mark.parametrize("dim", [20, 48, 136, 400])
@pytest.mark.parametrize("kind", ["gauss", "cancel", "ints"])
def test_matches_the_chain_oracle(gpu_pkg, monkeypatch, kind, dim):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    base, q, ri, rd = _data(kind, dim)
    if kind == "cancel":
        cancel_data.require(rd, 15, f"f16 filter dim {dim}")
    with gpu_pkg.BruteForceIndex.from_f16(base, id_offset=1000) as idx:
        for nb, B, k in SHAPES:
            _check(idx, q, ri, rd, nb, B, k, (kind, dim), 1000)
        st = idx.filter_stats()
        print("filter_stats", kind, dim, st)
        assert st[0] >= len(SHAPES) and st[1] == 0 and st[2] >= st[3] >= 1, st


def test_many_slabs(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    base, q, ri, rd = _data("gauss", 2048, 36)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        _check(idx, q, ri, rd, 4, 4, 15, "2048")
        _check(idx, q, ri, rd, 9, 4, 1, "2048")
        st = idx.filter_stats()
        assert st[0] >= 2 and st[1] == 0, st


def test_subnormals_and_the_range_end(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    base, q, ri, rd = _data("reals", 136, 128)
    raw = base.view(np.uint16)
    assert (((raw & 0x7C00) == 0) & ((raw & 0x03FF) != 0)).sum() >= 100 and (np.abs(base.astype(np.float32)) > 5.9e4).any()
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        _check(idx, q, ri, rd, 4, 32, 15, "reals")
        _check(idx, q, ri, rd, 9, 5, 1, "reals")
        assert idx.filter_stats()[0] == 2


def test_inner_product(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    rng = np.random.default_rng(5)
    base, q = rng.standard_normal((N, 48)).astype(np.float16), rng.standard_normal((20, 48)).astype(np.float32)
    with gpu_pkg.BruteForceIndex.from_f16(base, metric=gpu_pkg.METRIC_IP) as idx:
        _check(idx, q, *_ip_lists(q, base.astype(np.float32), 16), 4, 5, 15, "ip gauss")
        assert idx.filter_stats()[:2] == (1, 0)
    # integers; half of every query and the other half of most rows are zero: products exactly zero come back as -0.0
    base = rng.integers(-3, 4, size=(N, 20)).astype(np.float32)
    base[8:, 10:] = 0
    q = rng.integers(-3, 0, size=(128, 20)).astype(np.float32)
    q[:, :10] = 0
    ri, rd = _ip_lists(q[:20], base, 16)
    assert (cancel_data.bits(rd) == np.int32(-2 ** 31)).any()
    with gpu_pkg.BruteForceIndex.from_f16(base.astype(np.float16), metric=gpu_pkg.METRIC_IP) as idx:
        _check(idx, q, ri, rd, 4, 5, 15, "ip zero")
        assert idx.filter_stats()[0] == 1


@functools.lru_cache(maxsize=None)
def _width_lists(metric):
    """_data("gauss", 48) with, under inner product, the lists of the 85 queries that 17 batches of 5 use"""
    base, q, ri, rd = _data("gauss", 48)
    if metric == "ip":
        ri, rd = _ip_lists(q[:85], base.astype(np.float32), 16)
        ri.setflags(write=False), rd.setflags(write=False)
    return base, q, ri, rd


@pytest.mark.parametrize("nb", [6, 16, 17])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_every_sweep_width_and_two_passes(gpu_pkg, monkeypatch, metric, nb):
    """the sweep at 2 and 4 column blocks per wave (6 and 16 batches), and at 3 over two passes whose last block is partly
    dead (17 batches: 34 column blocks on 2 x 24); SHAPES runs 1 and 3 in one pass only"""
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    base, q, ri, rd = _width_lists(metric)
    with gpu_pkg.BruteForceIndex.from_f16(base, metric=gpu_pkg.METRIC_IP if metric == "ip" else gpu_pkg.METRIC_L2) as idx:
        _check(idx, q, ri, rd, nb, 5, 15, (metric, nb))
        assert idx.filter_stats()[:2] == (1, 0)  # the sweep, not the fallback, produced the result


@pytest.mark.parametrize("how", ["all rows equal", "a query value above 65504"])
def test_overflow_takes_the_fallback(gpu_pkg, monkeypatch, how):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "2")
    base, q, ri, rd = _data("same" if how == "all rows equal" else "gauss", 48, 128)
    if how != "all rows equal":
        q = q.copy()
        q[40, 9] = 7.0e4  # float16 cannot hold it: E = +inf for this query
        ri, rd = cancel_data.sorted_scores(q, base.astype(np.float32), 16)
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        _check(idx, q, ri, rd, 4, 32, 15, how)
        assert idx.filter_stats()[1] >= 1


@pytest.mark.parametrize("how", ["toggle", "an infinite half"])
def test_no_route(gpu_pkg, monkeypatch, how):
    monkeypatch.setenv("VSEARCH_ND_F16_FILTER", "0" if how == "toggle" else "2")
    base, q, ri, rd = _data("gauss", 48)
    if how != "toggle":
        base = base.copy()
        base[123, 7] = np.inf
    with gpu_pkg.BruteForceIndex.from_f16(base) as idx:
        assert idx.getNumDocs() == N
        if how == "toggle":
            _check(idx, q, ri, rd, 4, 32, 15, how)
        else:  # (an infinite distance is not this file's business: only that the index exists and keeps the old route)
            _dev(idx, q, 4, 32, 15)
        assert idx.filter_stats()[0] == 0
