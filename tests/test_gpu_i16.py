"""GPU checks of the int16 cosine runner (vs_i16_*): stored rows, score matrices and top-k, every one bit for bit.

The reference is numpy, written out here from the contract in include/vsearch.h: the one-line quantiser of the
reference's preprocess.py on float32 rows, then int64 products.  The result is exact integers, so there is no tolerance
anywhere: the device image must equal the quantiser, the score matrix q'.astype(int64) @ b'.astype(int64).T, and the
top-k np.lexsort((ids, -scores))."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N0 = 4099  # 64 full groups of 64 rows and a ragged one of 3
DIMS = [1, 7, 8, 9, 127, 128, 129, 136, 257, 960, 2047, 2048]
INT32_MIN = -(2 ** 31)


def quant(x, scale):
    """preprocess.py:24-42 on float32 rows (numpy's pairwise norm is the order the contract states)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return ((x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)) * np.float32(scale)).astype(np.int16)


def scores_ref(qq, bq):
    s = qq.astype(np.int64) @ bq.astype(np.int64).T
    assert np.abs(s).max(initial=0) < 2 ** 23
    return s


def topk_ref(s, k, id_offset=0):
    """Largest score first, equal scores in ascending id; slots past the rows are (-1, INT32_MIN)."""
    nq, n = s.shape
    ids = np.full((nq, k), -1, dtype=np.int32)
    top = np.full((nq, k), INT32_MIN, dtype=np.int64)
    rows = np.arange(n)
    for i in range(nq):
        cand = rows
        if n > 8192:  # only rows at or above the k-th largest score can appear: rank those
            cand = np.flatnonzero(s[i] >= np.partition(s[i], n - k)[n - k])
        order = cand[np.lexsort((cand, -s[i][cand]))[:k]]
        ids[i, : len(order)] = order + id_offset
        top[i, : len(order)] = s[i, order]
    return ids, top.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(n, dim, scale=1000.0):
    """(base, 70 queries, quantised base, quantised queries, int64 scores): real-valued rows, computed once, read-only."""
    rng = np.random.default_rng(100003 * dim + n)
    base = (rng.standard_normal((n, dim)) * rng.uniform(0.01, 30.0, size=(n, 1))).astype(np.float32)
    q = (rng.standard_normal((70, dim)) * rng.uniform(0.01, 30.0, size=(70, 1))).astype(np.float32)
    bq, qq = quant(base, scale), quant(q, scale)
    s = scores_ref(qq, bq)
    for a in (base, q, bq, qq, s):
        a.setflags(write=False)
    return base, q, bq, qq, s


@pytest.mark.parametrize("dim", DIMS)
def test_rows_and_score_matrix_over_dimensions(gpu_pkg, dim):
    base, q, bq, qq, s = _case(N0, dim)
    assert np.array_equal(gpu_pkg.i16_quantize(base), bq)
    with gpu_pkg.I16Runner(base) as r:
        assert (r.getNumDocs(), r.getDim(), r.getBatchSize(), r.getScale()) == (N0, dim, 32, 1000.0)
        assert np.array_equal(r.rows(), bq)
        assert np.array_equal(r.rows(4000, 99), bq[4000:])
        with pytest.raises(gpu_pkg.VSearchError) as e:
            r.rows(4000, 100)
        assert e.value.status == -1
        got = r.execute(q[:32])
    assert got.dtype == np.int32 and got.shape == (32, N0)
    assert np.array_equal(got, s[:32])


@pytest.mark.parametrize("scale", [1.0, 2047.0])
def test_rows_at_other_scales_and_special_rows(gpu_pkg, scale):
    base, _, _, _, _ = _case(N0, 257)
    base = base[:200].copy()
    base[3] = 0.0
    base[4] = 1e-42
    base[5, 7] = np.nan
    base[6, 9] = 1e30
    base[7, 11] = np.inf
    want = gpu_pkg.i16_quantize(base, scale)
    assert not want[3].any() and not want[5].any() and not want[6].any() and not want[7].any()
    with gpu_pkg.I16Runner(base, scale) as r:
        assert np.array_equal(r.rows(), want)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_few_rows(gpu_pkg, n):
    base, q, _, _, s = _case(n, 136)
    with gpu_pkg.I16Runner(base) as r:
        assert np.array_equal(r.execute(q[:32]), s[:32])


@pytest.mark.parametrize("dim", [136, 2048])
@pytest.mark.parametrize("B", [1, 16, 17, 31, 32])
def test_short_batches(gpu_pkg, dim, B):
    """B <= 16 takes the kernel with one query block, B > 16 the one with two; rows past B are zero queries."""
    base, q, _, _, s = _case(N0, dim)
    with gpu_pkg.I16Runner(base) as r:
        got = r.execute(q[:B])
    assert got.shape == (B, N0) and np.array_equal(got, s[:B])


@pytest.mark.parametrize("B,ld", [(5, N0 + 1), (32, N0 + 13), (17, N0), (32, 4112)])
def test_execute_dev_leading_dimension_and_stream(gpu_pkg, B, ld):
    """ld > rows and unaligned (scalar stores), aligned (16-byte stores), on a stream of the caller's own."""
    import torch

    base, q, _, _, s = _case(N0, 129)
    qd = torch.from_numpy(q[:B].copy()).cuda()
    stream = torch.cuda.Stream()
    with gpu_pkg.I16Runner(base) as r:
        for shift in (0, 1):  # shift 1: the output pointer itself is not 16-byte aligned
            buf = torch.full((B * ld + 8,), -77, dtype=torch.int32, device="cuda")
            out = buf[shift:]
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                r.execute_dev(qd.data_ptr(), B, out.data_ptr(), ld, stream.cuda_stream)
            stream.synchronize()
            got = out[: B * ld].cpu().numpy().reshape(B, ld)
            assert np.array_equal(got[:, :N0], s[:B])
            assert (got[:, N0:] == -77).all() and (buf[shift + B * ld:] == -77).all()  # nothing written past a row's end


@functools.lru_cache(maxsize=None)
def _adversarial():
    """2048-d rows at scale 2047: self-matches near scale^2, alternating signs whose partial sums run up before they
    cancel, and rows of +-1-level components."""
    dim, scale = 2048, 2047.0
    rng = np.random.default_rng(2048)
    rows = []
    spike = np.zeros((8, dim), np.float32)  # one or two dominant components: quantised values up to 2047
    for i in range(8):
        spike[i, 37 * i] = 5.0
        spike[i, 37 * i + 1] = 0.02 * i
    rows.append(spike)
    few = np.zeros((64, dim), np.float32)  # a few large components of mixed sign
    for i in range(64):
        idx = rng.choice(dim, size=2 + i % 7, replace=False)
        few[i, idx] = rng.choice([-1.0, 1.0], size=len(idx)) * rng.uniform(0.5, 1.0, size=len(idx))
    rows.append(few)
    # sign patterns by row % 4: strictly alternating | first half +, second half - | all + | both.  An all + query against
    # a half / half row: the running sum climbs to scale^2 / 2 and comes back to nearly 0
    alt = rng.uniform(0.9, 1.1, size=(64, dim)).astype(np.float32)
    alternating = np.where(np.arange(dim) % 2 == 0, 1.0, -1.0).astype(np.float32)
    halves = np.where(np.arange(dim) < dim // 2, 1.0, -1.0).astype(np.float32)
    alt[0::4] *= alternating
    alt[1::4] *= halves
    alt[3::4] *= alternating * halves
    rows.append(alt)
    ones = rng.uniform(-1, 1, size=(64, dim))  # a quarter of the components large, the others quantise to +-1
    unit = np.linalg.norm(ones[:, : dim // 4], axis=1, keepdims=True) / scale
    ones[:, dim // 4:] = rng.choice([-1.0, 1.0], size=(64, dim - dim // 4)) * rng.uniform(1.1, 1.9, size=(64, dim - dim // 4)) * unit
    rows.append(ones.astype(np.float32))
    rows.append(rng.standard_normal((4099 - 200, dim)).astype(np.float32))
    base = np.concatenate(rows)
    q = np.concatenate([spike[:4], few[:8], alt[:12], ones[:8]])  # queries that are base rows
    bq, qq = quant(base, scale), quant(q, scale)
    s = scores_ref(qq, bq)
    assert s.max() > 0.99 * scale * scale and np.abs(bq).max() == 2047 and (np.abs(bq[136:200, dim // 4:]) == 1).all()
    run = np.cumsum(qq[14].astype(np.int64) * bq[73].astype(np.int64))  # the all + row against a half / half row
    assert run.max() > 0.4 * scale * scale and abs(run[-1]) < 0.05 * scale * scale and run[-1] == s[14, 73]
    for a in (base, q, s):
        a.setflags(write=False)
    return base, q, s, scale


def test_adversarial_scores_and_topk(gpu_pkg):
    base, q, s, scale = _adversarial()
    with gpu_pkg.I16Runner(base, scale) as r:
        got = r.execute(q)
        ids, top = r.search(q, 16)
    assert np.array_equal(got, s)
    wi, wt = topk_ref(s, 16)
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


@pytest.mark.parametrize("k", [1, 5, 8, 9, 16])
def test_topk_host_call_with_ragged_last_batch(gpu_pkg, k):
    base, q, _, _, s = _case(N0, 136)
    with gpu_pkg.I16Runner(base, id_offset=1000) as r:
        ids, top = r.search(q, k)  # 70 queries: two batches of 32 and one of 6
    wi, wt = topk_ref(s, k, 1000)
    assert ids.dtype == np.int32 and top.dtype == np.int32 and ids.shape == (70, k)
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


@pytest.mark.parametrize("dim", [1, 9, 960, 2047])
def test_topk_over_dimensions(gpu_pkg, dim):
    """At 1-d every score is +-scale^2 or 0: thousands of ties, all resolved by ascending id."""
    base, q, _, _, s = _case(N0, dim)
    with gpu_pkg.I16Runner(base) as r:
        ids, top = r.search(q[:40], 10)
    wi, wt = topk_ref(s[:40], 10)
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


@pytest.mark.parametrize("B,nb,k", [(32, 2, 10), (7, 3, 16), (16, 4, 5), (17, 18, 8)])
def test_search_dev_batches_on_a_stream(gpu_pkg, B, nb, k):
    """Several batches per launch (18 batches: two launch groups), short batches, a stream of the caller's own."""
    import torch

    base, q, _, qq, s = _case(N0, 257)
    sel = np.arange(nb * B) % 70
    qd = torch.from_numpy(q[sel].copy()).cuda()
    ids = torch.full((nb * B, k), -7, dtype=torch.int32, device="cuda")
    top = torch.zeros((nb * B, k), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with gpu_pkg.I16Runner(base, id_offset=5) as r:
        with torch.cuda.stream(stream):
            r.search_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    wi, wt = topk_ref(s[sel], k, 5)
    assert np.array_equal(top.cpu().numpy(), wt) and np.array_equal(ids.cpu().numpy(), wi)


def test_duplicates_across_a_group_boundary(gpu_pkg):
    """Copies of one row at ids 60..67 (both sides of the 64-row boundary) and 4090..4098: equal scores, ascending id."""
    base, q, _, _, _ = _case(N0, 136)
    base = base.copy()
    base[60:68] = base[10]
    base[4090:4099] = base[10]
    qs = np.concatenate([base[10:11], q[:20]])
    s = scores_ref(quant(qs, 1000.0), quant(base, 1000.0))
    with gpu_pkg.I16Runner(base) as r:
        ids, top = r.search(qs, 16)
    wi, wt = topk_ref(s, 16)
    assert list(wi[0]) == [10] + list(range(60, 68)) + list(range(4090, 4097))
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


@pytest.mark.parametrize("n", [1, 5, 15])
def test_fewer_rows_than_k(gpu_pkg, n):
    base, q, _, _, s = _case(n, 136)
    with gpu_pkg.I16Runner(base) as r:
        ids, top = r.search(q[:33], 16)
    wi, wt = topk_ref(s[:33], 16)
    assert (wi[:, n:] == -1).all() and (wt[:, n:] == INT32_MIN).all()
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)


def test_threshold_exchange_path(gpu_pkg):
    """Enough rows that every wave has blocks left after its first one: the scan exchanges bounds between workgroups.
    8-d rows with many near-duplicates keep the ties in play."""
    n = 64 * 8 * 256 * 4 + 37
    rng = np.random.default_rng(8)
    base = rng.standard_normal((n, 8)).astype(np.float32)
    base[rng.integers(0, n, 4000)] = base[123]
    q = np.concatenate([base[123:124], rng.standard_normal((63, 8)).astype(np.float32)])
    s = scores_ref(quant(q, 1000.0), quant(base, 1000.0))
    with gpu_pkg.I16Runner(base) as r:
        ids, top = r.search(q, 16)
        ids5, top5 = r.search(q[:16], 5)
    wi, wt = topk_ref(s, 16)
    assert np.array_equal(top, wt) and np.array_equal(ids, wi)
    assert np.array_equal(top5, wt[:16, :5]) and np.array_equal(ids5, wi[:16, :5])


def test_argument_limits(gpu_pkg):
    import ctypes as C

    base, q, _, _, _ = _case(65, 136)
    L = gpu_pkg.lib()
    with gpu_pkg.I16Runner(base) as r:
        with pytest.raises(gpu_pkg.VSearchError) as e:
            r.search(q, 17)
        assert e.value.status == -5
        with pytest.raises(gpu_pkg.VSearchError) as e:
            r.search(q, 0)
        assert e.value.status == -1
        p = q.ctypes.data_as(C.c_void_p)
        assert L.vs_i16_execute(r._h, p, 33, p) == -1 and L.vs_i16_execute(r._h, p, 0, p) == -1
        assert L.vs_i16_execute_dev(r._h, p, 4, p, 64, None) == -1  # ld < rows
        assert L.vs_i16_search_dev(r._h, p, 1, 33, 5, p, p, None) == -1
        assert L.vs_i16_search_dev(r._h, p, 1, 4, 17, p, p, None) == -5
