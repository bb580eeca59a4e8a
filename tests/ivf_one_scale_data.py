"""Data of the two-launch route's tests at nlist = 1024 (a plain helper module like ivf_ip_data.py and near_ties.py):
tests/test_ivf_one_scale_host.py asserts every precondition on the CPU, tests/test_gpu_ivf_one_scale.py runs the device.

The integer index.  Values are integers in [0, 256) with 2 dim 255^2 < 2^24 (`_hi` of test_gpu_ivf_nd.py), so every coarse
score and every distance is exact in fp32 in any summation order.  Two dimensions: 100 (dim_p = 112, seven 16-float
segments) and 40.  nd_dim_p(20) / 16 = 2 is EVEN, so the twin below 128 is dim 40: dim_p = 48, three segments -- the half
step of ivf_one_block_dots runs at both.  The query fragments take dim_p 64 = 7168 and 3072 bytes, less than the selection's
won table (8192 bytes), which is therefore the larger overlay of the coarse launch's first LDS region at both dimensions.

  centroids : 16 groups of 64 around integer anchors, given explicitly (they are not the lists' means: planting a row never
              moves a probe).  GROUP_OF spreads a group's list ids by a fixed random permutation, so the probes of a query
              that sits on an anchor land in many lanes of the selection (lane = id & 63) and in several register slots
              (id >> 6) of one lane, never in a contiguous id range.
  lists     : SHAPED = sizes 0, 1, 63, 64, 65, 511, 512, 513 and the hot list of 3100 rows (7 units of 512); every other
              list holds 4 to 12 rows; the last list is not empty and ends at row N (about 13 000).
  duplicates: PAIRS = four pairs (lo, hi) of lists whose centroids are bit-identical: (a, a + 64) one lane and neighbouring
              slots, (a', a' + 960) one lane and slots 0 and 15, (b, b + 1) neighbouring lanes, (c, c + 513) on opposite
              sides of the unit table's two-lists-per-thread ownership.  Both lists of a pair belong to one group.  The
              higher list holds an exact copy of the centroid (at its row PLANT_ROW), the lower list does not, and the sizes
              differ.
  queries   : three sets of 16.  groups: anchor i plus noise.  hot: the hot list's centroid moved 25 to 40 % of the way to
              another group's anchor, a different group per query.  dups: the pairs' centroids (each four times).
"""
import functools

import numpy as np

import near_ties
import oracle
from test_gpu_ivf_nd import _hi

NLIST = 1024
GROUPS, PER_GROUP = 16, 64
DIMS = (100, 40)
UNIT = 512  # rows per unit of the scan (ivf_one_plan(...)[2]; the GPU file asserts it)
HOT, HOT_ROWS = 40, 3100
SHAPED = {3: 0, 5: 1, 7: 63, 8: 64, 9: 65, 500: 511, 511: 512, 600: 513, HOT: HOT_ROWS}
EMPTY = 3
PAIRS = ((70, 70 + 64), (37, 37 + 960), (300, 301), (200, 200 + 513))
PAIR_SIZES = (6, 11)  # rows of the lower and of the higher list of every pair
PLANT_ROW = 2         # the higher list's row that is the centroid itself
MASK_QUERIES = (1, 6, 11)  # the hot set's queries of planted_index


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=1)
def group_of():
    """[NLIST] the group of every list: a fixed random spread, then both lists of every pair put into one group"""
    rng = np.random.default_rng(41000)
    g = rng.permutation(np.repeat(np.arange(GROUPS), PER_GROUP))
    fixed = {i for p in PAIRS for i in p} | set(SHAPED)
    for lo, hi in PAIRS:
        if g[hi] == g[lo]:
            continue
        x = next(int(i) for i in np.nonzero(g == g[lo])[0] if int(i) not in fixed)  # a member of lo's group trades places with hi
        g[x], g[hi] = g[hi], g[lo]
    assert np.all(np.bincount(g, minlength=GROUPS) == PER_GROUP)
    return _freeze(g)[0]


def list_sizes():
    rng = np.random.default_rng(41001)
    sizes = rng.integers(4, 13, size=NLIST)
    for c, n in SHAPED.items():
        sizes[c] = n
    for lo, hi in PAIRS:
        sizes[lo], sizes[hi] = PAIR_SIZES
    return sizes


@functools.lru_cache(maxsize=2)
def int_index(dim):
    """(vectors_reordered, centroids, offsets, reorder_to_original, anchors), read-only and shared between tests"""
    assert _hi(dim) == 256
    rng = np.random.default_rng(41100 + dim)
    g = group_of()
    anchors = rng.integers(30, 226, size=(GROUPS, dim))
    cents = anchors[g] + rng.integers(-4, 5, size=(NLIST, dim))
    for lo, hi in PAIRS:
        cents[hi] = cents[lo]
    sizes = list_sizes()
    off = np.zeros(NLIST + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    vr = np.clip(np.repeat(cents, sizes, axis=0) + rng.integers(-8, 9, size=(n, dim)), 0, 255)
    for lo, hi in PAIRS:
        rows = vr[off[lo]:off[lo + 1]]
        same = (rows == cents[lo]).all(1)
        rows[same, 0] += 1  # (never taken in practice: the lower list holds no copy of the centroid)
        vr[off[hi] + PLANT_ROW] = cents[hi]
    r2o = rng.permutation(n).astype(np.int32)
    return _freeze(np.ascontiguousarray(vr, dtype=np.float32), cents.astype(np.float32), off, r2o, anchors.astype(np.float32))


@functools.lru_cache(maxsize=2)
def query_sets(dim):
    """{"groups", "hot", "dups"}: [16, dim] each"""
    vr, cents, off, r2o, anchors = int_index(dim)
    rng = np.random.default_rng(41200 + dim)
    groups = np.clip(anchors + rng.integers(-2, 3, size=anchors.shape), 0, 255).astype(np.float32)
    g_hot = int(group_of()[HOT])
    others = [g for g in range(GROUPS) if g != g_hot]
    hot = np.empty((16, dim), dtype=np.float32)
    for i in range(16):
        t = (0.25, 0.30, 0.35, 0.40)[i % 4]
        to = anchors[others[i % len(others)]] - cents[HOT]
        hot[i] = np.clip(cents[HOT] + np.rint(t * to) + rng.integers(-1, 2, size=dim), 0, 255)
    dups = np.stack([cents[PAIRS[i % 4][0]] for i in range(16)]).astype(np.float32)
    return dict(zip(("groups", "hot", "dups"), _freeze(groups, hot, dups)))


def first_lists(data, nlist):
    """the index of the first nlist lists: rows, centroids and offsets cut, ids renumbered in their order"""
    vr, cents, off, r2o = data[:4]
    n = int(off[nlist])
    ids = np.argsort(np.argsort(r2o[:n], kind="stable"), kind="stable").astype(np.int32)
    return (np.ascontiguousarray(vr[:n]), np.ascontiguousarray(cents[:nlist]), np.ascontiguousarray(off[:nlist + 1]), ids)


def last_lists_queries(cents, nlist):
    """16 queries on the centroids of lists nlist - 1, nlist - 2, ...: the highest register slots that hold a list at this
    nlist are probed whatever the other sets do (at nlist = 513 list 512 is the only entry of its slot)"""
    return np.ascontiguousarray(cents[nlist - 16:nlist][::-1], dtype=np.float32)


@functools.lru_cache(maxsize=2)
def signed_variant(dim):
    """The index and its query sets moved to [-127, 127] as ivf_ip_data.signed_index's values are (dim 127^2 < 2^24:
    every product is exact): scores of both signs for the inner-product case.  The pairs stay bit-identical."""
    assert dim * 127 * 127 < 2 ** 24
    vr, cents, off, r2o, _ = int_index(dim)
    move = lambda a: np.clip(a - 128.0, -127, 127).astype(np.float32)
    q = np.concatenate([move(query_sets(dim)[s]) for s in ("groups", "hot", "dups")])
    return _freeze(move(vr), move(cents), off, r2o, q)


@functools.lru_cache(maxsize=1)
def planted_index(dim):
    """A copy of the hot set's query j (j in MASK_QUERIES) in every list of at least three rows that another query of the
    batch probes at nprobe = 256 and j does not; behind the list's row 64 where the list is that long.
    Returns (vectors_reordered, {j: (planted lists, planted positions)})."""
    vr, cents, off, r2o, _ = int_index(dim)
    q = query_sets(dim)["hot"]
    probes = oracle.ivf_search(vr, off, r2o, cents, q, 1, 256, return_probes=True)[3]
    sizes = np.diff(off)
    vr = np.array(vr)
    planted = {}
    for t, j in enumerate(MASK_QUERIES):
        mine = set(probes[j].tolist())
        theirs = set(np.delete(probes, j, axis=0).ravel().tolist()) - mine
        lists = [c for c in sorted(theirs) if sizes[c] >= 3]
        rows = [int(off[c]) + (64 + t if sizes[c] > 64 + t else int(sizes[c]) - 1 - t) for c in lists]
        vr[rows] = q[j]
        planted[j] = (np.array(lists), np.array(rows))
    return _freeze(vr)[0], planted


@functools.lru_cache(maxsize=1)
def one_vector_index(dim):
    """the index with every row the same vector: every distance of a query is equal"""
    vr = np.empty_like(int_index(dim)[0])
    vr[:] = np.arange(dim) % 7 + 100
    return _freeze(vr)[0]


@functools.lru_cache(maxsize=1)
def one_more_list(dim):
    """the index with a list of 9 rows appended: nlist = 1025"""
    vr, cents, off, r2o, _ = int_index(dim)
    rng = np.random.default_rng(41300 + dim)
    c = rng.integers(30, 226, size=(1, dim)).astype(np.float32)
    rows = np.clip(c + rng.integers(-8, 9, size=(9, dim)), 0, 255).astype(np.float32)
    n = len(vr)
    return _freeze(np.concatenate([vr, rows]), np.concatenate([cents, c]), np.append(off, n + 9).astype(np.int32),
                   np.append(r2o, np.arange(n, n + 9)).astype(np.int32))


GAUSS_NPROBE = 16


@functools.lru_cache(maxsize=1)
def gauss_index():
    """Non-integer data at nlist = 1024, dim 100: 32 clusters of 32 centroids, centre N(0, 1), centroid = centre + N(0, 0.05^2),
    4 to 12 rows = centroid + N(0, 0.05^2) per list; 32 ordinary queries near the centres and 300 forced coarse near-ties
    at nprobe = 16 (near_ties.boundary_queries): a query near a centre has its 16th and 17th centroid inside one cluster,
    both close to it, which is where the summation order of q.c decides the probe set (tests/test_gpu_ivf_nd.py,
    _gauss_index).  Returns (vectors_reordered, centroids, offsets, reorder_to_original, queries, forced queries, mask)."""
    dim = 100
    rng = np.random.default_rng(41400)
    centres = rng.normal(0, 1, size=(32, dim))
    cl = rng.permutation(np.repeat(np.arange(32), 32))
    cents = (centres[cl] + 0.05 * rng.normal(0, 1, size=(NLIST, dim))).astype(np.float32)
    sizes = rng.integers(4, 13, size=NLIST)
    off = np.zeros(NLIST + 1, dtype=np.int32)
    off[1:] = np.cumsum(sizes)
    n = int(off[-1])
    vr = (np.repeat(cents.astype(np.float64), sizes, axis=0) + 0.05 * rng.normal(0, 1, size=(n, dim))).astype(np.float32)
    r2o = rng.permutation(n).astype(np.int32)
    q = (centres + 0.02 * rng.normal(0, 1, size=centres.shape)).astype(np.float32)
    seeds = centres[rng.integers(0, 32, size=300)] + 0.02 * rng.normal(0, 1, size=(300, dim))
    fq, mask = near_ties.boundary_queries(cents, seeds, GAUSS_NPROBE, rng)
    return _freeze(vr, cents, off, r2o, q, fq, mask)


def units_of(off, probes, unit=UNIT):
    """the unit table's length for a batch with these probes: every probed list that holds rows, cut into units"""
    sizes = np.diff(off)[np.unique(probes)]
    return int(((sizes + unit - 1) // unit).sum())
