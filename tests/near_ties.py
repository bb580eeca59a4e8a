"""Queries that sit on a coarse near-tie, shared by the IVF tests (a plain helper module like nd_u8_data.py).

An ordinary query's coarse scores at ranks nprobe and nprobe + 1 differ by far more than fp32 rounding, so the order in
which a dot product is summed never decides its probe set and a test on ordinary queries cannot tell a kernel with the
wrong accumulation order, a norm that is off in the last bits or a selection that misorders nearly equal scores from a
right one.  boundary_queries() moves every seed query onto the hyperplane on which those two scores are EQUAL and then
off it by a few units in the last place: there the summation order decides, and the oracle's two orders ("lanes8", the
reference's stand-in, and "chain", the product's fp32 MFMA kernels) disagree about the probe set for a large share of
the queries.  A test that demands the chain oracle's result for every one of them pins the device's arithmetic bit for
bit; require_teeth() asserts, on the CPU and before the device is called, that the share is large enough to do so.

The queries are not rounded to integers (rounding removes the ties): on a byte-valued index their batches take the fp32
rows, which is the path whose arithmetic is in question.
"""
import numpy as np

import oracle


def coarse_scores(cents, q, dot_order, metric=0):
    """[nq, nlist] coarse scores as the oracle's IVF search forms them: fmaf(-2, q.c, |q|^2 + |c|^2), or for the inner
    product -2 q.c (the oracle ranks by -q.c; the factor 2 is exact and keeps the order)."""
    cents = np.ascontiguousarray(cents, dtype=np.float32)
    q = np.ascontiguousarray(q, dtype=np.float32)
    if metric == 0:
        return oracle.l2_matrix(q, cents, dot_order)
    zero = np.zeros(len(cents), dtype=np.float32)
    out = np.empty((len(q), len(cents)), dtype=np.float32)
    for i in range(len(q)):  # (l2_row takes the query's norm from the query: hand it the row-wise call with both norms 0)
        oracle.lib().vo_l2_row_order(q[i], 0.0, cents, zero, len(cents), cents.shape[1], oracle.DOT_ORDERS[dot_order], out[i])
    return out


def probe_lists(cents, q, nprobe, dot_order, metric=0):
    """the oracle's probes: the nprobe smallest scores by (score, list id), as lists and the scores that go with them"""
    s = coarse_scores(cents, q, dot_order, metric)
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), s), axis=1)[:, :nprobe]
    return order, np.take_along_axis(s, order, 1)


def boundary_queries(cents, q0, nprobe, rng, metric=0, tmax=1e-6, rounds=6, ulps=1.0):
    """For every seed query of q0: a and b = the centroids at ranks nprobe and nprobe + 1 (float64 scores), the query moved
    along a - b onto the set where both score alike (L2: the bisecting hyperplane of a and b; inner product: the
    hyperplane q.(a - b) = 0), plus t (a - b) with |t| <= tmax (see below), cast to fp32.
    Returns (queries fp32 [nq, dim], mask [nq]: the probe SETS of the lanes8 and the chain oracle differ)."""
    c = np.asarray(cents, dtype=np.float64)
    x = np.array(q0, dtype=np.float64)
    assert 1 <= nprobe < len(c), "no boundary: every list is probed"
    # Moving a query onto the hyperplane of its pair changes its other scores too, and where many centroids are about
    # equally far (unclustered data) another centroid may come between the two: repeat with the pair that is at the
    # boundary now, a few times (a step moves a query less and less; whatever pair is last decides).
    for _ in range(rounds):
        if metric == 0:
            s = (x ** 2).sum(1)[:, None] - 2 * x @ c.T + (c ** 2).sum(1)[None]
        else:
            s = -(x @ c.T)
        rank = np.argsort(s, axis=1, kind="stable")
        a, b = c[rank[:, nprobe - 1]], c[rank[:, nprobe]]
        ab = a - b
        n2 = (ab ** 2).sum(1)
        assert (n2 > 0).all(), "two centroids coincide: their scores are equal everywhere, not nearly equal"
        if metric == 0:
            along = ((x - 0.5 * (a + b)) * ab).sum(1) / n2
        else:
            along = (x * ab).sum(1) / n2
        x = x - along[:, None] * ab
    # t moves the difference of the two scores by 2 t |a - b|^2 (inner product: t |a - b|^2).  Where that is many units in
    # the last place of a score (centroids far apart for their size) no rounding can bridge it: cap |t| per query so that
    # the two scores stay within `ulps` units in the last place of each other, and never above tmax.
    if metric == 0:
        size = (x ** 2).sum(1) + (a ** 2).sum(1)
        cap = ulps * 2.0 ** -23 * size / (2 * n2)
    else:
        size = np.abs((x * a).sum(1))
        cap = ulps * 2.0 ** -23 * size / n2
    t = rng.uniform(-1, 1, size=len(x)) * np.minimum(tmax, cap)
    q = (x + t[:, None] * ab).astype(np.float32)
    pa, _ = probe_lists(cents, q, nprobe, "lanes8", metric)
    pb, _ = probe_lists(cents, q, nprobe, "chain", metric)
    mask = np.array([set(pa[i].tolist()) != set(pb[i].tolist()) for i in range(len(q))])
    return q, mask


def require_teeth(mask, label):
    """The condition that gives a forced-tie test its teeth (not a tolerance): for at least a tenth of the forced queries,
    and at least 20 of them, the probe set depends on the summation order.  Prints the share."""
    share = float(mask.mean())
    print(f"[near-ties] {label}: probe set depends on the dot order for {int(mask.sum())} of {len(mask)} forced queries ({100 * share:.1f} %)")
    assert mask.sum() >= 20 and share >= 0.10, (label, int(mask.sum()), len(mask))
    return share


def describe(cents, q, i, nprobe, metric=0):
    """what to print when query i differs from the chain oracle: the query, both oracles' probe lists and the two coarse
    scores at the first rank where the lists differ"""
    pa, sa = probe_lists(cents, q[i:i + 1], nprobe, "lanes8", metric)
    pb, sb = probe_lists(cents, q[i:i + 1], nprobe, "chain", metric)
    diff = np.nonzero(pa[0] != pb[0])[0]
    r = int(diff[0]) if len(diff) else -1
    with np.printoptions(precision=9, threshold=4096, linewidth=160):
        txt = (f"query {i}:\n{q[i]!r}\nprobes lanes8: {pa[0].tolist()}\nprobes chain : {pb[0].tolist()}\n")
        if r >= 0:
            txt += (f"first differing rank {r}: lanes8 list {pa[0][r]} score {float(sa[0][r])!r} ({sa[0][r:r + 1].view(np.int32)[0]:#x}), "
                    f"chain list {pb[0][r]} score {float(sb[0][r])!r} ({sb[0][r:r + 1].view(np.int32)[0]:#x})")
        else:
            txt += "the two oracles pick the same probes in the same order"
    return txt
