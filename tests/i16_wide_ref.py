"""numpy reference of the int16 cosine runner's wide top-k (vs_i16_search_topk*), shared by its host and GPU tests.

Written out from the contract in include/vsearch.h: the one-line quantiser of the reference's preprocess.py on float32
rows, int64 products, np.lexsort((ids, -scores)); the sampling rule of vs_i16_wide_plan and, from it, the number of
candidates a query has (rows whose score is at least the k-th best score of the sample), which decides the path a shape
takes.  Everything is exact integers: no tolerance anywhere."""
import functools

import numpy as np

INT32_MIN = -(2 ** 31)
CAP = 8192
N1 = 20483  # 320 full groups of 64 rows and a ragged one of 3


def quant(x, scale=1000.0):
    """preprocess.py:24-42 on float32 rows (numpy's pairwise norm is the order the contract states)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return ((x / (np.linalg.norm(x, axis=1, keepdims=True) + 1e-8)) * np.float32(scale)).astype(np.int16)


def scores_ref(qq, bq):
    """The int64 products q'.b'.  Computed in float64, where they are the same numbers (every product is below 2^22 and
    every sum of at most 2048 of them below 2^53, so nothing is rounded) and the matrix product is quick; a few rows are
    computed again in int64 to say so."""
    s = (qq.astype(np.float64) @ bq.astype(np.float64).T).astype(np.int64)
    rows = np.unique(np.linspace(0, bq.shape[0] - 1, 7).astype(np.int64))
    assert np.array_equal(s[:, rows], qq.astype(np.int64) @ bq[rows].astype(np.int64).T)
    assert np.abs(s).max(initial=0) < 2 ** 23
    return s


def expected_stats(s, k, batches):
    """vs_i16_wide_stats after one call on an index whose counters were zero: `batches` is the list of batch sizes the call
    makes, in query order.  A batch with a query of more than CAP candidates is answered by the dense fallback."""
    counts = cand_counts(s, k)
    assert sum(batches) == s.shape[0]
    if counts is None:
        return (0, 0, 0, s.shape[0])
    ranked = dense = q0 = 0
    for b in batches:
        if counts[q0:q0 + b].max() > CAP:
            dense += b
        else:
            ranked += b
        q0 += b
    return (ranked, int(counts.max()), dense, 0)


def host_batches(nq):
    """The batches of the host call: full batches of 32, then the short last one."""
    return [32] * (nq // 32) + ([nq % 32] if nq % 32 else [])


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


def plan_ref(n_rows, k):
    """(sample groups, stride, cap): the rule of vs_i16_wide_plan, restated."""
    n_groups = -(-n_rows // 64)
    l0 = max(64 * k, -(-n_rows * k // 2048))
    sample_groups = min(n_groups, -(-l0 // 64))
    return sample_groups, n_groups // sample_groups, CAP


def sample_rows(n_rows, k):
    """The sampled rows, and whether the sample is the whole base."""
    sg, stride, _ = plan_ref(n_rows, k)
    n_groups = -(-n_rows // 64)
    if sg == n_groups:
        return np.arange(n_rows), True
    rows = (np.arange(sg)[:, None] * stride * 64 + np.arange(64)[None, :]).ravel()
    assert rows.max() < n_rows - n_rows % 64 and len(rows) >= 64 * k  # full groups only
    return rows, False


def cand_counts(s, k):
    """Per query: the rows with a score >= the k-th best score of the sample (None when the sample is the whole base)."""
    rows, whole = sample_rows(s.shape[1], k)
    if whole:
        return None
    sub = s[:, rows]
    kth = np.partition(sub, sub.shape[1] - k, axis=1)[:, sub.shape[1] - k]
    return (s >= kth[:, None]).sum(axis=1)


@functools.lru_cache(maxsize=None)
def case(n, dim, scale=1000.0, nq=70):
    """(base, queries, int64 scores): the gaussian rows of tests/test_gpu_i16.py::_case, computed once, read-only."""
    rng = np.random.default_rng(100003 * dim + n)
    base = (rng.standard_normal((n, dim)) * rng.uniform(0.01, 30.0, size=(n, 1))).astype(np.float32)
    q = (rng.standard_normal((70, dim)) * rng.uniform(0.01, 30.0, size=(70, 1))).astype(np.float32)[:nq]
    s = scores_ref(quant(q, scale), quant(base, scale))
    for a in (base, q, s):
        a.setflags(write=False)
    return base, q, s


@functools.lru_cache(maxsize=None)
def adversarial():
    """The adversarial set of tests/test_gpu_i16.py, restated: 2048-d rows at scale 2047 with self-matches near scale^2,
    alternating signs whose partial sums run up before they cancel, and rows of +-1-level components."""
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
    assert s.max() > 0.99 * scale * scale and np.abs(bq).max() == 2047
    for a in (base, q, s):
        a.setflags(write=False)
    return base, q, s, scale
