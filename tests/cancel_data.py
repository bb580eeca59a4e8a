"""Real-valued rows on which squared-L2 distances cancel, shared by test_oracle.py and test_gpu_cancel.py (a plain helper
module like near_ties.py).

Every kernel forms d = fmaf(-2, q.b, |q|^2 + |b|^2) with q.b summed in the MFMA "chain" order and the norms in the
8-lane order.  Where a query IS a row the three terms cancel and what is left is rounding noise: a small number of
either sign, or exactly +0.  cancel_data() makes such queries on Gaussian rows, with duplicate rows far apart in row
order (bit-equal distances: the tie flag fires and the replay runs on distances that are no integers) and two planted
neighbours per query at small distances that are NOT noise.  The chain oracle restates the kernels bit for bit, so a
test on this data needs no tolerance; counts() says, on the reference alone, how many queries do what the data is for.
"""
import numpy as np

import oracle

TRIPLE = 50  # rows 0 .. 49 exist three times

# Every data set of test_gpu_cancel.py as (rows, self-queries, dim, offset of the rows' mean); test_oracle.py asserts on
# the reference alone, for each of them, that it produces what it is for.  Seeds are SEED + dim (100 + dim left 3 exact
# zeros among the coarse scores of the 100-d IVF sets, below the floor of 4; 101 + dim clears every floor).
SEED = 101
BF_SETS = [(20000, 640, 128, 0), (20000, 640, 128, 4), (3000, 48, 128, 0), (3000, 48, 128, 4), (66000, 128, 128, 4),
           (30000, 128, 128, 0), (30000, 128, 128, 4)] + [(20000, 96, dim, offset) for dim in (20, 100, 384) for offset in (0, 4)]
# (rows, self-queries, dim, offset, lists)
IVF_SETS = [(20000, 96, 128, 0, 64), (20000, 96, 128, 4, 64), (20000, 96, 128, 0, 5000)] + \
           [(6000, 64, dim, offset, 24) for dim in (20, 100) for offset in (0, 4)]
_CACHE = {}


def layout(n):
    """(m, mid): rows [n - m, n) copy rows [0, m); rows [mid, mid + TRIPLE) copy rows [0, TRIPLE).  mid is no multiple of
    64, so a copy never sits at its original's place inside a 64-row block."""
    m = n // 10
    mid = (n // 2 // 64) * 64 + 37
    return m, mid


def cancel_data(rng, n, nq, dim, offset):
    """base [n, dim], queries [nq, dim] (float32) and src [nq]: query i is row src[i] bit for bit.  The first
    min(nq // 4, TRIPLE) queries are rows of a triple.  Query i has two planted neighbours, rows m + 3 i + 1 (the query
    times 1 + 2^-12) and n - m - 2 - 5 i (the query plus 2^-10 times a unit vector)."""
    m, mid = layout(n)
    assert m >= TRIPLE + nq and m + 3 * nq + 1 < mid and n - m - 2 - 5 * nq >= mid + TRIPLE, (n, nq)
    base = (rng.standard_normal((n, dim)) + offset).astype(np.float32)
    nt = min(nq // 4, TRIPLE)
    src = np.concatenate([rng.choice(TRIPLE, nt, replace=False), TRIPLE + rng.choice(m - TRIPLE, nq - nt, replace=False)])
    q = base[src].copy()
    u = rng.standard_normal((nq, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    i = np.arange(nq)
    base[m + 3 * i + 1] = q * np.float32(1 + 2.0 ** -12)
    base[n - m - 2 - 5 * i] = (q.astype(np.float64) + 2.0 ** -10 * u).astype(np.float32)
    base[n - m:] = base[:m]
    base[mid:mid + TRIPLE] = base[:TRIPLE]
    return base, q, src.astype(np.int64)


def cancel_ivf_layout(base, nlist, rng, prefer=None):
    """Centroids = nlist distinct rows with distinct values, taken from the rows `prefer` first (the self-queries' rows:
    such a query's coarse score at its own centroid cancels too) and from the rows before the last block of copies for
    the rest; every row in the list of its nearest centroid by the chain oracle's score (equal scores: the lower list),
    lists in the stable reordered layout.  Returns (vectors_reordered, offsets, reorder_to_original, centroids)."""
    n = len(base)
    m, mid = layout(n)
    first = np.unique(np.asarray(prefer, dtype=np.int64))[:nlist] if prefer is not None else np.zeros(0, dtype=np.int64)
    pool = np.setdiff1d(np.arange(n - m), np.concatenate([first, np.arange(mid, mid + TRIPLE)]))
    rows = np.sort(np.concatenate([rng.permutation(first), rng.choice(pool, nlist - len(first), replace=False)]))
    cents = base[rows].copy()
    assert len(np.unique(cents, axis=0)) == nlist
    score = oracle.l2_matrix(cents, base, "chain")  # [nlist, n]; a score is symmetric in its two vectors, bit for bit
    assign = score.argmin(0)
    order = np.argsort(assign, kind="stable").astype(np.int32)
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    return np.ascontiguousarray(base[order]), off, order, cents


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def case(n, nq, dim, offset):
    """cancel_data(default_rng(SEED + dim), ...), made once and read-only"""
    key = (n, nq, dim, offset)
    if key not in _CACHE:
        _CACHE[key] = _frozen(*cancel_data(np.random.default_rng(SEED + dim), n, nq, dim, offset))
    return _CACHE[key]


def ivf_case(n, nq, dim, offset, nlist):
    """(vectors_reordered, offsets, reorder_to_original, centroids, queries) over case()'s rows: the layout continues the
    same generator, its centroids are rows of self-queries first"""
    key = (n, nq, dim, offset, nlist)
    if key not in _CACHE:
        rng = np.random.default_rng(SEED + dim)
        base, q, src = cancel_data(rng, n, nq, dim, offset)
        vr, off, r2o, cents = cancel_ivf_layout(base, nlist, rng, prefer=src)
        _CACHE[key] = _frozen(vr, off, r2o, cents, ivf_queries(q, cents))
    return _CACHE[key]


def ivf_queries(q, cents):
    """the self-queries plus nlist // 2 queries that are centroids, bit for bit"""
    return np.ascontiguousarray(np.concatenate([q, cents[::2][:len(cents) // 2]]))


def sorted_scores(q, base, k1, dot_order="chain"):
    """k1 best of every query by (distance, row id) ascending from the chain score matrix: (ids int32, distances)"""
    s = oracle.l2_matrix(q, base, dot_order)
    o = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), s), axis=1)[:, :k1]
    return o.astype(np.int32), np.take_along_axis(s, o, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def counts(d, k):
    """d [nq, >= k + 1]: ascending distances.  Queries with (a negative best distance, an exact +0 inside the top k, two
    equal distances inside the k + 1 best, a negative k-th best distance)."""
    d = np.asarray(d, dtype=np.float32)
    zero = (d[:, :k] == 0) & ~np.signbit(d[:, :k])
    return (int((d[:, 0] < 0).sum()), int(zero.any(1).sum()), int(((d[:, :k] == d[:, 1:k + 1]) & np.isfinite(d[:, :k])).any(1).sum()),
            int((d[:, k - 1] < 0).sum()))


def require(d, k, label, negative=1, zero=1, tie=1):
    """what keeps a test on this data from passing vacuously: the expected arrays hold a negative distance, a +0 and a tie"""
    c = counts(d, k)
    print(f"[cancel] {label}: of {len(d)} queries {c[0]} have a negative best distance, {c[1]} a +0 in their top {k}, "
          f"{c[2]} a tie inside their {k + 1} best, {c[3]} a negative bound (min {float(np.min(d)):.3g})")
    assert c[0] >= negative and c[1] >= zero and c[2] >= tie, (label, c)
    return c
