"""GPU checks of the int16 cosine runner's top-k up to k = 128 (vs_i16_search_topk*), every one bit for bit.

The reference is tests/i16_wide_ref.py: the numpy quantiser line, int64 products, np.lexsort((ids, -scores)).  A test
that is about a path first asserts that path's precondition on the CPU (the candidates per query that follow from
vs_i16_wide_plan: all at most the cap for the list path, some above it for the dense fallback), and every test compares
vs_i16_wide_stats with what the CPU expects; on the list path the largest candidate count must match exactly."""
import functools

import numpy as np
import pytest

import i16_wide_ref as ref
from i16_wide_ref import CAP, INT32_MIN, N1

pytestmark = pytest.mark.gpu


def check_host(pkg, base, q, s, k, scale=1000.0, id_offset=0, runner=None):
    """One host call on a fresh (or reset) runner: exact ids and scores, and the counters the CPU expects.  Returns them."""
    want_stats = ref.expected_stats(s, k, ref.host_batches(len(q)))
    wi, wt = ref.topk_ref(s, k, id_offset)
    r = runner or pkg.I16Runner(base, scale, id_offset=id_offset)
    try:
        r.wide_stats(reset=True)
        ids, top = r.search_topk(q, k)
        stats = r.wide_stats(reset=True)
        assert r.wide_stats() == (0, 0, 0, 0)
    finally:
        if runner is None:
            r.close()
    assert ids.dtype == np.int32 and top.dtype == np.int32 and ids.shape == (len(q), k) and top.shape == (len(q), k)
    assert np.array_equal(top, wt)
    assert np.array_equal(ids, wi)
    assert stats == want_stats
    return stats


def device_call(r, qd, nb, B, k, stream, guard=64):
    """search_topk_dev into fresh buffers with guard words behind them; nothing is synchronised here."""
    import torch

    ids = torch.full((nb * B * k + guard,), -7, dtype=torch.int32, device="cuda")
    top = torch.full((nb * B * k + guard,), -9, dtype=torch.int32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())  # the fills above
    with torch.cuda.stream(stream):
        r.search_topk_dev(qd.data_ptr(), nb, B, k, ids.data_ptr(), top.data_ptr(), stream.cuda_stream)
    return ids, top


def device_result(ids, top, nb, B, k):
    n = nb * B * k
    assert (ids[n:] == -7).all() and (top[n:] == -9).all()  # nothing written behind the outputs
    return ids[:n].cpu().numpy().reshape(nb * B, k), top[:n].cpu().numpy().reshape(nb * B, k)


@pytest.mark.parametrize("dim", [7, 128, 136, 960, 2048])
def test_dimensions_on_the_list_path(gpu_pkg, dim):
    base, q, s = ref.case(N1, dim)
    assert ref.cand_counts(s, 100).max() <= CAP
    stats = check_host(gpu_pkg, base, q, s, 100)  # two full batches and a batch of 6
    assert stats[0] == 70 and stats[2] == 0 and stats[3] == 0


@pytest.mark.parametrize("k", [17, 32, 33, 64, 100, 128])
def test_k_sweep(gpu_pkg, k):
    base, q, s = ref.case(N1, 136)
    assert ref.cand_counts(s, k).max() <= CAP
    stats = check_host(gpu_pkg, base, q, s, k)
    assert stats[0] == 70 and stats[2] == 0


@pytest.mark.parametrize("k", [5, 16])
def test_small_k_is_the_fused_call(gpu_pkg, k):
    import torch

    base, q, s = ref.case(N1, 136)
    with gpu_pkg.I16Runner(base, id_offset=3) as r:
        ids, top = r.search_topk(q, k)
        ids0, top0 = r.search(q, k)
        assert np.array_equal(ids, ids0) and np.array_equal(top, top0)
        qd = torch.from_numpy(q[:64].copy()).cuda()
        out = [torch.zeros((64, k), dtype=torch.int32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        s0 = torch.cuda.current_stream().cuda_stream
        r.search_topk_dev(qd.data_ptr(), 2, 32, k, out[0].data_ptr(), out[1].data_ptr(), s0)
        r.search_dev(qd.data_ptr(), 2, 32, k, out[2].data_ptr(), out[3].data_ptr(), s0)
        torch.cuda.synchronize()
        assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])
        assert np.array_equal(out[0].cpu().numpy(), ids0[:64])
        assert r.wide_stats() == (0, 0, 0, 0)  # no wide call was made
    wi, wt = ref.topk_ref(s, k, 3)
    assert np.array_equal(ids, wi) and np.array_equal(top, wt)


@pytest.mark.parametrize("B", [1, 16, 17, 32])
def test_device_call_on_a_stream(gpu_pkg, B):
    """18 batches: two launch groups; short batches have padding queries; a stream of the caller's own."""
    import torch

    nb, k = 18, 40
    base, q, s = ref.case(N1, 136)
    sel = np.arange(nb * B) % 70
    want_stats = ref.expected_stats(s[sel], k, [B] * nb)
    assert want_stats[2] == 0 and want_stats[0] == nb * B
    qd = torch.from_numpy(q[sel].copy()).cuda()
    stream = torch.cuda.Stream()
    with gpu_pkg.I16Runner(base, id_offset=5) as r:
        ids, top = device_call(r, qd, nb, B, k, stream)
        stream.synchronize()
        stats = r.wide_stats()
    gi, gt = device_result(ids, top, nb, B, k)
    wi, wt = ref.topk_ref(s[sel], k, 5)
    assert np.array_equal(gt, wt) and np.array_equal(gi, wi)
    assert stats == want_stats


def test_calls_back_to_back_without_a_sync(gpu_pkg):
    """k = 100, k = 20 and k = 100 again on one stream, nothing waited for in between: the counters of a call are cleared
    in stream order behind the call before it."""
    import torch

    base, q, s = ref.case(N1, 136)
    qd = torch.from_numpy(q[:64].copy()).cuda()
    stream = torch.cuda.Stream()
    with gpu_pkg.I16Runner(base) as r:
        outs = [device_call(r, qd, 2, 32, k, stream) for k in (100, 20, 100)]
        stream.synchronize()
        stats = r.wide_stats()
    res = [device_result(i, t, 2, 32, k) for (i, t), k in zip(outs, (100, 20, 100))]
    for (gi, gt), k in zip(res, (100, 20, 100)):
        wi, wt = ref.topk_ref(s[:64], k)
        assert np.array_equal(gt, wt) and np.array_equal(gi, wi)
    assert np.array_equal(res[0][0], res[2][0]) and np.array_equal(res[0][1], res[2][1])
    c100, c20 = ref.cand_counts(s[:64], 100), ref.cand_counts(s[:64], 20)
    assert stats == (192, max(c100.max(), c20.max()), 0, 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_few_rows(gpu_pkg, n):
    base, q, s = ref.case(n, 136)
    stats = check_host(gpu_pkg, base, q, s, 128)
    assert stats == (0, 0, 0, 70)  # the sample is the whole base for every query
    wi, wt = ref.topk_ref(s, 128)
    m = min(n, 128)
    assert (wi[:, m:] == -1).all() and (wt[:, m:] == INT32_MIN).all() and (wi[:, :m] >= 0).all()


def _first_sampled(k):
    """The smallest n_rows whose sample is not the whole base."""
    n = 64 * k + 1
    assert ref.plan_ref(n, k)[0] < -(-n // 64) and ref.plan_ref(n - 1, k)[0] == -(-(n - 1) // 64)
    return n


@pytest.mark.parametrize("k,n", [(17, 1088), (17, 1089), (17, 1152), (17, 1153)] +
                         [(100, _first_sampled(100) + d) for d in (0, 1, 64)])
def test_around_the_sample_boundary(gpu_pkg, k, n):
    base, q, s = ref.case(n, 136)
    stats = check_host(gpu_pkg, base, q, s, k)
    whole = n <= 64 * k
    assert (stats[3] == 70) == whole and (stats[0] == 70) == (not whole)


def test_mass_ties_one_dimension(gpu_pkg):
    """1-d rows: every score is +-scale^2 or 0, about half the base ties at the top: every list overflows."""
    base, q, s = ref.case(N1, 1)
    for k in (17, 100):
        assert ref.cand_counts(s, k).min() > CAP
        stats = check_host(gpu_pkg, base, q, s, k)
        assert stats[2] == 70 and stats[0] == 0


@functools.lru_cache(maxsize=None)
def _copies():
    """12 000 copies of one row among N1 136-d rows; 32 queries next to that row, then 38 queries orthogonal to it."""
    base, q, _ = ref.case(N1, 136)
    rng = np.random.default_rng(12000)
    base = base.copy()
    row = base[77].copy()
    base[rng.choice(N1, 12000, replace=False)] = row
    u = row / np.linalg.norm(row)
    near = (row[None, :] + 0.05 * np.linalg.norm(row) / np.sqrt(136) * rng.standard_normal((32, 136))).astype(np.float32)
    far = q[:38] - (q[:38].astype(np.float64) @ u)[:, None] * u[None, :]
    qs = np.concatenate([near, far.astype(np.float32)])
    s = ref.scores_ref(ref.quant(qs), ref.quant(base))
    return base, qs, s


def test_mass_ties_copies_of_one_row(gpu_pkg):
    base, qs, s = _copies()
    counts = ref.cand_counts(s, 100)
    assert counts[:32].min() > CAP and counts[32:].max() <= CAP
    stats = check_host(gpu_pkg, base, qs, s, 100)
    assert stats[2] == 32 and stats[0] == 38 and stats[1] > 12000


@functools.lru_cache(maxsize=None)
def _zeros(n):
    """All but 40 rows are zero rows or have a support disjoint from the queries': their scores are exactly 0."""
    rng = np.random.default_rng(40 + n)
    base = np.zeros((n, 136), np.float32)
    other = rng.choice(n, n // 2, replace=False)
    base[other, 68:] = rng.standard_normal((len(other), 68)).astype(np.float32)
    live = rng.choice(n, 40, replace=False)
    base[live] = 0
    base[live, :68] = rng.standard_normal((40, 68)).astype(np.float32)
    q = np.zeros((70, 136), np.float32)
    q[:, :68] = rng.standard_normal((70, 68)).astype(np.float32)
    s = ref.scores_ref(ref.quant(q), ref.quant(base))
    assert (np.count_nonzero(s, axis=1) <= 40).all() and (s > 0).any() and (s < 0).any()
    wi, wt = ref.topk_ref(s, 100)
    assert (wt[:, 99] == 0).all() and (wt[:, 0] > 0).all()  # the k-th best is exactly 0; ties run by id
    return base, q, s


@pytest.mark.parametrize("n", [8000, N1])
def test_zero_at_the_kth_place(gpu_pkg, n):
    """8000 rows: every row at or above 0 is a candidate and they fit the cap (the bound is next_up(-0.0) on the list
    path); N1 rows: they do not (the fallback)."""
    import torch

    base, q, s = _zeros(n)
    counts = ref.cand_counts(s, 100)
    assert counts.max() <= CAP if n == 8000 else counts.min() > CAP
    with gpu_pkg.I16Runner(base) as r:
        stats = check_host(gpu_pkg, base, q, s, 100, runner=r)
        assert (stats[0], stats[2]) == ((70, 0) if n == 8000 else (0, 70))
        # B = 5: 27 padding queries per batch, zero queries that score 0 everywhere and must list nothing
        nb, B = 3, 5
        qd = torch.from_numpy(q[:nb * B].copy()).cuda()
        stream = torch.cuda.Stream()
        ids, top = device_call(r, qd, nb, B, 100, stream)
        stream.synchronize()
        stats = r.wide_stats()
    gi, gt = device_result(ids, top, nb, B, 100)
    wi, wt = ref.topk_ref(s[:nb * B], 100)
    assert np.array_equal(gt, wt) and np.array_equal(gi, wi)
    assert stats == ref.expected_stats(s[:nb * B], 100, [B] * nb)


@pytest.mark.parametrize("k", [17, 100])
def test_ordered_base(gpu_pkg, k):
    """Rows sorted by their score to query 0, best last: a prefix sample would bound nothing, the strided one does."""
    base, q, s = ref.case(N1, 136)
    order = np.argsort(s[0], kind="stable")
    base, s = base[order], s[:, order]
    assert (np.diff(s[0]) >= 0).all() and ref.cand_counts(s, k).max() <= CAP
    stats = check_host(gpu_pkg, base, q, s, k)
    assert stats[0] == 70 and stats[2] == 0


def test_adversarial(gpu_pkg):
    base, q, s, scale = ref.adversarial()
    check_host(gpu_pkg, base, q, s, 64, scale=scale)


def test_id_offset(gpu_pkg):
    base, q, s = ref.case(N1, 136)
    check_host(gpu_pkg, base, q, s, 50, id_offset=1000000)


def test_large_base(gpu_pkg):
    """524 325 8-d rows: a full grid, stride 20 at k = 100."""
    n = 524325
    rng = np.random.default_rng(n)
    base = rng.standard_normal((n, 8)).astype(np.float32)
    q = rng.standard_normal((70, 8)).astype(np.float32)
    s = ref.scores_ref(ref.quant(q), ref.quant(base))
    assert gpu_pkg.i16_wide_plan(n, 100)[:2] == (401, 20)
    with gpu_pkg.I16Runner(base) as r:
        for k in (17, 100):
            assert ref.cand_counts(s, k).max() <= CAP
            stats = check_host(gpu_pkg, base, q, s, k, runner=r)
            assert stats[0] == 70 and stats[2] == 0


def test_limits(gpu_pkg):
    import ctypes as C

    base, q, _ = ref.case(65, 136)
    L = gpu_pkg.lib()
    with gpu_pkg.I16Runner(base) as r:
        for k, status in ((0, -1), (-3, -1), (129, -5)):
            with pytest.raises(gpu_pkg.VSearchError) as e:
                r.search_topk(q, k)
            assert e.value.status == status
        p = q.ctypes.data_as(C.c_void_p)
        assert L.vs_i16_search_topk_dev(r._h, p, 1, 4, 0, p, p, None) == -1
        assert L.vs_i16_search_topk_dev(r._h, p, 1, 4, 129, p, p, None) == -5
        assert L.vs_i16_search_topk_dev(r._h, p, 1, 33, 129, p, p, None) == -1  # B before k
        assert L.vs_i16_search_topk_dev(r._h, p, 0, 4, 100, p, p, None) == -1
        assert L.vs_i16_search_topk_dev(r._h, None, 1, 4, 100, p, p, None) == -1
        assert L.vs_i16_search_topk(r._h, p, -1, 100, p, p) == -1
        assert r.wide_stats() == (0, 0, 0, 0)
