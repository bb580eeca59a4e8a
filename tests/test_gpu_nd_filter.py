"""bf16 prefilter of a general fp32 index: search_dev_multi under VSEARCH_ND_FILTER=2 against the lists ranked
by (distance, id) from the chain oracle -- ids, distance bits and flags -- on real-valued rows (E > 0), on self-queries over
duplicated rows (distances cancel and tie) and on SIFT-like integers; inner product, overflow, an ill-scaled base, the
toggle, and the row image against numpy."""
import functools

import numpy as np
import pytest

import cancel_data
import oracle

pytestmark = pytest.mark.gpu

N = 4096 + 37
SHAPES = [(nb, B, k) for nb in (4, 9) for B in (32, 5) for k in (1, 15)]


@functools.lru_cache(maxsize=None)
def _data(kind, dim, nq=288, pkg=None):
    """(base, queries, ids [nq, 16], distances [nq, 16]) made once and read-only"""
    rng = np.random.default_rng(77 + dim)
    if kind == "gauss":
        base, q = rng.standard_normal((N, dim)).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32)
    elif kind == "cancel":
        base, q, _ = cancel_data.cancel_data(rng, N, nq, dim, 4)
    elif kind == "same":
        base, q = np.tile(rng.standard_normal((1, dim)).astype(np.float32), (N, 1)), rng.standard_normal((nq, dim)).astype(np.float32)
    else:
        base, q = pkg.synth_sift(N, 5, dim), pkg.synth_sift(nq, 6, dim)
    ri, rd = cancel_data.sorted_scores(q, base, 16)
    for a in (base, q, ri, rd):
        a.setflags(write=False)
    return base, q, ri, rd


def _dev(idx, q, nb, B, k):
    import torch
    n = nb * B
    qd = torch.from_numpy(np.array(q[:n])).cuda()
    oi = torch.full((n, k + 1), -7, dtype=torch.int32, device="cuda")
    od = torch.full((n, k + 1), 7.0, dtype=torch.float32, device="cuda")
    fl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    idx.search_dev_multi(qd.data_ptr(), nb, B, k, oi.data_ptr(), od.data_ptr(), fl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy(), od.cpu().numpy(), fl.cpu().numpy()


def _check(idx, q, ri, rd, nb, B, k, tag, id_offset=0):
    gi, gd, fl = _dev(idx, q, nb, B, k)
    wi, wd = ri[:nb * B, :k + 1] + id_offset, rd[:nb * B, :k + 1]
    assert np.array_equal(gi, wi), (tag, nb, B, k, "ids", np.nonzero((gi != wi).any(1))[0][:8])
    assert np.array_equal(cancel_data.bits(gd), cancel_data.bits(wd)), (tag, nb, B, k, "distance bits")
    assert np.array_equal(fl, (wd[:, :-1] == wd[:, 1:]).any(1).astype(np.int32)), (tag, nb, B, k, "flags")


@pytest.mark.parametrize("dim", [20, 48, 136, 400])
@pytest.mark.parametrize("kind", ["gauss", "cancel", "sift"])
def test_matches_the_chain_oracle(gpu_pkg, monkeypatch, kind, dim):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    base, q, ri, rd = _data(kind, dim, 288, gpu_pkg if kind == "sift" else None)
    if kind == "cancel":
        cancel_data.require(rd, 15, f"nd filter dim {dim}")
    with gpu_pkg.BruteForceIndex(base, id_offset=1000) as idx:
        for nb, B, k in SHAPES:
            _check(idx, q, ri, rd, nb, B, k, (kind, dim), 1000)
        st = idx.filter_stats()
        assert st[0] >= len(SHAPES) and st[1] == 0 and st[2] >= st[3] >= 1, st


def test_many_slabs(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    base, q, ri, rd = _data("gauss", 2048, 36)
    with gpu_pkg.BruteForceIndex(base) as idx:
        _check(idx, q, ri, rd, 4, 4, 15, "2048")
        _check(idx, q, ri, rd, 9, 4, 1, "2048")
        st = idx.filter_stats()
        assert st[0] >= 1 and st[1] == 0, st


def _ip_lists(q, base, k1):
    s = np.array([[-oracle.dot(b, x, "chain") for b in base] for x in q], dtype=np.float32)
    o = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), s), axis=1)[:, :k1]
    return o.astype(np.int32), np.take_along_axis(s, o, 1)


def test_inner_product(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    rng = np.random.default_rng(5)
    base, q = rng.standard_normal((N, 48)).astype(np.float32), rng.standard_normal((20, 48)).astype(np.float32)
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP) as idx:
        _check(idx, q, *_ip_lists(q, base, 16), 4, 5, 15, "ip gauss")
        assert idx.filter_stats()[:2] == (1, 0)
    # integers; half of every query and the other half of most rows are zero: products exactly zero come back as -0.0
    base = rng.integers(-3, 4, size=(N, 20)).astype(np.float32)
    base[8:, 10:] = 0
    q = rng.integers(-3, 0, size=(128, 20)).astype(np.float32)
    q[:, :10] = 0
    ri, rd = _ip_lists(q[:20], base, 16)
    assert (cancel_data.bits(rd) == np.int32(-2 ** 31)).any()
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP) as idx:
        _check(idx, q, ri, rd, 4, 5, 15, "ip zero")


@functools.lru_cache(maxsize=None)
def _width_lists(metric):
    """_data("gauss", 48) with, under inner product, the lists of the 85 queries that 17 batches of 5 use"""
    base, q, ri, rd = _data("gauss", 48)
    if metric == "ip":
        ri, rd = _ip_lists(q[:85], base, 16)
        ri.setflags(write=False), rd.setflags(write=False)
    return base, q, ri, rd


@pytest.mark.parametrize("nb", [6, 16, 17])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_every_sweep_width_and_two_passes(gpu_pkg, monkeypatch, metric, nb):
    """the sweep at 2 and 4 column blocks per wave (6 and 16 batches), and at 3 over two passes whose last block is partly
    dead (17 batches: 34 column blocks on 2 x 24); SHAPES runs 1 and 3 in one pass only"""
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    base, q, ri, rd = _width_lists(metric)
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP if metric == "ip" else gpu_pkg.METRIC_L2) as idx:
        _check(idx, q, ri, rd, nb, 5, 15, (metric, nb))
        assert idx.filter_stats()[:2] == (1, 0)  # the sweep, not the fallback, produced the result


def test_overflow_takes_the_fallback(gpu_pkg, monkeypatch):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    base, q, ri, rd = _data("same", 48, 128)
    with gpu_pkg.BruteForceIndex(base) as idx:
        _check(idx, q, ri, rd, 4, 32, 15, "same")
        assert idx.filter_stats()[1] >= 1


@pytest.mark.parametrize("how", ["ill scaled", "toggle"])
def test_no_image_keeps_the_old_route(gpu_pkg, monkeypatch, how):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "0" if how == "toggle" else "2")
    base, q, ri, rd = _data("gauss", 48)
    if how == "ill scaled":
        base = base.copy()
        base[123, 7] = 1e30
        ri, rd = cancel_data.sorted_scores(q[:128], base, 16)
    with gpu_pkg.BruteForceIndex(base) as idx:
        with pytest.raises(Exception):
            idx.filter_image(0, 1)
        _check(idx, q, ri, rd, 4, 32, 15, how)


@pytest.mark.parametrize("dim", [20, 136])
def test_image_is_bf16_rne_in_row_order(gpu_pkg, monkeypatch, dim):
    monkeypatch.setenv("VSEARCH_ND_FILTER", "2")
    base = _data("gauss", dim)[0]
    u = base.view(np.uint32).astype(np.uint64)
    want = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)  # round to nearest even (no NaN here)
    with gpu_pkg.BruteForceIndex(base) as idx:
        got = idx.filter_image(0, N + 64)
    assert got.shape == (N + 64, (dim + 31) // 32 * 32)
    assert np.array_equal(got[:N, :dim], want) and not got[:N, dim:].any() and not got[N:].any()
