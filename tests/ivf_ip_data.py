"""Data of the inner-product IVF tests (a plain helper module like near_ties.py and nd_u8_data.py).

Every set uses the list cuts of tests/test_gpu_ivf_nd.py: N = 6000 rows in 24 lists, one empty, one of 1 row, lists of 63,
64 and 65 rows, one of 1200 rows, and the last list ends at row N (its last 64-row block reads the spare rows behind the
index).  All values are integers small enough that every product q.v and q.c is exact in fp32 in any summation order, so
the tests assert equality with oracle.ivf_search(..., metric=1) for every query.

  signed_index(dim)   : rows and queries in [-a, a] with dim a^2 < 2^24; scores of both signs.  Query 4 equals the empty
                        list's centroid, a vector of +-a no other centroid comes near: the empty list is its best list.
  negative_index(dim) : rows in [1, hi), clustered around one centre per list (high everywhere but on a few coordinates of
                        the list's own), and queries = -(a vector of the rows' kind),
                        so every product is negative and every score s = -(q.v) is positive.  A row past a list's end
                        -- the next list's rows, or the zero spare rows, which score -0.0 -- would beat every real row:
                        the set that catches a missing row mask.  Queries 0..3 are built to prefer the 1-row, the 63-row
                        and the 65-row list and the last list.
  zeros_index()       : signed_index(20) with rows planted orthogonal to queries 1 and 2, and queries 0 and 5 all zero:
                        scores that are exactly -0.0, beside positive and negative ones.
"""
import functools
import math

import numpy as np

from test_gpu_ivf_nd import EMPTY, N, NLIST, SHAPED, _nearest

NQ = 70
ONE_ROW, ROWS63, ROWS65, LAST = 5, 7, 9, NLIST - 1
assert SHAPED[ONE_ROW] == 1 and SHAPED[ROWS63] == 63 and SHAPED[ROWS65] == 65 and SHAPED[EMPTY] == 0


def amp(dim):
    """the largest a <= 127 with dim a^2 < 2^24"""
    a = min(int(math.isqrt((2 ** 24 - 1) // dim)), 127)
    assert a >= 1 and dim * a * a < 2 ** 24
    return a


def list_offsets():
    rest = N - sum(SHAPED.values())
    free = [c for c in range(NLIST) if c not in SHAPED]
    sizes = np.zeros(NLIST, dtype=np.int64)
    for c, n in SHAPED.items():
        sizes[c] = n
    for j, c in enumerate(free):
        sizes[c] = rest // len(free) + (1 if j < rest % len(free) else 0)
    off = np.zeros(NLIST + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    assert off[-1] == N and sizes[LAST] > 0
    return off


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=3)
def signed_index(dim):
    """(vectors_reordered, centroids, offsets, reorder_to_original, queries), read-only and shared between tests"""
    rng = np.random.default_rng(9000 + dim)
    a = amp(dim)
    base = rng.integers(-a, a + 1, size=(N, dim)).astype(np.float32)
    src = rng.integers(100, N - 100, size=40)
    base[:20] = base[src[:20]]  # duplicated rows: equal scores, ranked by position
    base[N - 20:] = base[src[20:]]
    q = rng.integers(-a, a + 1, size=(NQ, dim)).astype(np.float32)
    q[:4] = base[src[:4]]
    assign = _nearest(base, base[rng.choice(N, NLIST, replace=False)])
    order = np.argsort(assign, kind="stable")
    off = list_offsets()
    vr = np.ascontiguousarray(base[order])
    r2o = order.astype(np.int32)
    cents = np.zeros((NLIST, dim), dtype=np.float32)
    for c in range(NLIST):
        if off[c + 1] > off[c]:
            cents[c] = np.rint(vr[off[c]:off[c + 1]].astype(np.float64).mean(0))
    # the empty list's centroid: +-a everywhere; q.c = dim a^2 for the query on it, which no other centroid reaches
    v = (a * rng.choice([-1, 1], size=dim)).astype(np.float32)
    assert not any(np.array_equal(v, cents[c]) for c in range(NLIST) if c != EMPTY)
    cents[EMPTY] = v
    q[4] = v
    return _freeze(vr, cents, off, r2o, q)


def _hi_pos(dim):
    hi = min(int(math.isqrt((2 ** 24 - 1) // dim)) + 1, 256)
    assert dim * (hi - 1) ** 2 < 2 ** 24
    return hi


@functools.lru_cache(maxsize=2)
def negative_index(dim):
    rng = np.random.default_rng(9500 + dim)
    hi = _hi_pos(dim)
    off = list_offsets()
    # a list's centre is high everywhere but on a few coordinates of its own, where it is low
    m = max(2, dim // 5)
    low = [tuple(sorted(rng.choice(dim, m, replace=False).tolist())) for _ in range(NLIST)]
    assert len(set(low)) == NLIST
    centres = rng.integers(hi - 40, hi, size=(NLIST, dim))
    for c in range(NLIST):
        centres[c, list(low[c])] = rng.integers(1, 9, size=m)
    vr = np.empty((N, dim), dtype=np.float32)
    for c in range(NLIST):
        n = off[c + 1] - off[c]
        vr[off[c]:off[c + 1]] = np.clip(centres[c][None, :] + rng.integers(-3, 4, size=(n, dim)), 1, hi - 1)
    r2o = rng.permutation(N).astype(np.int32)
    cents = np.zeros((NLIST, dim), dtype=np.float32)
    for c in range(NLIST):
        if off[c + 1] > off[c]:
            cents[c] = np.rint(vr[off[c]:off[c + 1]].astype(np.float64).mean(0))
    cents[EMPTY] = centres[EMPTY]
    # a query that prefers list c: heavy where that list's centre is low, light elsewhere (q.c is the least negative there)
    want = [ONE_ROW, ROWS63, ROWS65, LAST] + [int(c) for c in rng.integers(0, NLIST, size=NQ - 4)]
    q = np.empty((NQ, dim), dtype=np.float32)
    for i, c in enumerate(want):
        w = rng.integers(1, 4, size=dim)
        w[list(low[c])] = hi - 1 - rng.integers(0, 3, size=m)
        q[i] = -w
    assert vr.min() >= 1 and q.max() <= -1
    return _freeze(vr, cents, off, r2o, q)


ZERO_QUERIES = (0, 5)
ORTH_QUERIES = (1, 2)
ORTH_COORDS = 4


@functools.lru_cache(maxsize=1)
def zeros_index():
    dim = 20
    vr, cents, off, r2o, q = signed_index(dim)
    vr, q = np.array(vr), np.array(q)
    rng = np.random.default_rng(9700)
    planted = np.sort(rng.choice(N, 300, replace=False))
    planted = np.concatenate([planted, [off[ONE_ROW], off[ROWS63 + 1] - 1, N - 1]])  # short lists and the last row too
    vr[planted, :ORTH_COORDS] = 0
    for i in ZERO_QUERIES:
        q[i] = 0
    for i in ORTH_QUERIES:
        q[i] = 0
        q[i, :ORTH_COORDS] = rng.choice([-3, -2, -1, 1, 2, 3], size=ORTH_COORDS)
    return _freeze(vr, cents, off, r2o, q) + (planted,)


@functools.lru_cache(maxsize=1)
def duplicates_index():
    """8500 copies of one row of +-a (the largest norm there is) in a 9000-row list, and query 2 equal to it: the copies
    are its best rows, all with one score, more than a candidate list holds -- the ranking takes the exact fallback"""
    rng = np.random.default_rng(9800)
    dim, nlist = 20, 8
    a = amp(dim)
    sizes = [9000] + [200] * 7
    n = sum(sizes)
    vr = rng.integers(-a, a + 1, size=(n, dim)).astype(np.float32)
    rep = (a * rng.choice([-1, 1], size=dim)).astype(np.float32)
    vr[300:8800] = rep
    assert int((vr == rep).all(1).sum()) == 8500
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    r2o = rng.permutation(n).astype(np.int32)
    cents = np.stack([np.rint(vr[off[c]:off[c + 1]].astype(np.float64).mean(0)) for c in range(nlist)]).astype(np.float32)
    q = rng.integers(-a, a + 1, size=(5, dim)).astype(np.float32)
    q[2] = rep
    return _freeze(vr, cents, off, r2o, q)


@functools.lru_cache(maxsize=2)
def gauss_index(dim):
    """N(0, 1) rows, n = 4000 in 24 lists (nearest of 24 sampled rows, float64), centroids = the lists' means in fp32;
    70 ordinary queries and 300 N(0, 1) seeds for the forced coarse near-ties (near_ties.boundary_queries, metric=1)"""
    rng = np.random.default_rng(9900 + dim)
    n, nlist = 4000, 24
    base = rng.normal(0, 1, size=(n, dim)).astype(np.float32)
    q = rng.normal(0, 1, size=(NQ, dim)).astype(np.float32)
    seeds = rng.normal(0, 1, size=(300, dim)).astype(np.float32)
    b64 = base.astype(np.float64)
    cen0 = b64[rng.choice(n, nlist, replace=False)]
    assign = ((b64 * b64).sum(1)[:, None] - 2 * b64 @ cen0.T + (cen0 * cen0).sum(1)[None, :]).argmin(1)
    order = np.argsort(assign, kind="stable")
    vr = np.ascontiguousarray(base[order])
    r2o = order.astype(np.int32)
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    assert np.all(np.diff(off) > 0)
    cents = np.stack([vr[off[c]:off[c + 1]].mean(0) for c in range(nlist)]).astype(np.float32)
    return _freeze(base, vr, cents, off, r2o, q, seeds)
