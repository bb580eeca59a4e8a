"""vs_topk_merge_dev restated in plain numpy from the contract in include/vsearch.h, the generator of its test inputs and
the route a query takes through the two merge kernels, computed on the CPU (tests/test_gpu_merge.py asserts the routes
as preconditions, tests/test_merge_host.py checks this file itself).

The contract: a list ends at its first entry whose distance is not < +inf or whose id is negative; the entries before
the ends are pooled per query and ordered by np.lexsort((ids, dists)) -- -0.0 == +0.0, ties by ascending id; the first
kout are the output, every distance with the bits of the entry it came from, the rest is (+inf, -1); the flag is 1 iff two
adjacent distances among the first min(kout, 256) outputs are equal and below +inf."""
import numpy as np

INF = np.float32(np.inf)
ID_MAX = 2 ** 31 - 2   # the largest id the contract allows (2^31 - 1 is taken as "none")
CAP = 4096             # vs_topk_merge_plan's out[1]: G*kin up to this runs the compacting kernel
TRACK = 256            # ... out[2]: the outputs among which the flag looks for a tie
KEEP = 512             # the compacting kernel's filter sets aside at most this many survivors
SUBNORMAL = np.float32(1e-40)
# the small set the generator draws distances from: either sign (the inner-product scores are negative), both zeros, a
# subnormal, values one ulp apart
VALUES = np.array([-np.inf, -1e30, -3.5, -1.0, -0.0, 0.0, SUBNORMAL, 0.5, np.nextafter(np.float32(0.5), INF), 1.0, 7.25,
                   3e38], dtype=np.float32)


def list_lengths(d, i):
    """d, i [..., kin] -> the number of entries before each list's end."""
    ended = ~(d < INF) | (i < 0)
    return np.where(ended.any(-1), ended.argmax(-1), d.shape[-1])


def merge_ref(d, i, kout):
    """d float32 [G, B, kin], i int32 [G, B, kin] -> (dists [B, kout] float32, ids [B, kout] int32, flags [B] int32,
    M [B]: the pooled entries per query)."""
    G, B, kin = d.shape
    lens = list_lengths(d, i)
    od = np.full((B, kout), INF, dtype=np.float32)
    oi = np.full((B, kout), -1, dtype=np.int32)
    fl = np.zeros(B, dtype=np.int32)
    live = np.arange(kin) < lens[:, :, None]  # [G, B, kin]
    for b in range(B):
        m = live[:, b, :]
        dists, ids = d[:, b, :][m], i[:, b, :][m]
        order = np.lexsort((ids, dists))[:kout]
        od[b, :len(order)] = dists[order]
        oi[b, :len(order)] = ids[order]
        w = od[b, :min(kout, TRACK)]
        fl[b] = 1 if np.any((w[:-1] == w[1:]) & (w[:-1] < INF)) else 0
    return od, oi, fl, lens.sum(0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the generator
def fill_query(rng, G, kin, M, values=VALUES, ends="mixed"):
    """One query: M entries with distances drawn from `values` and distinct ids (a permutation, 2^31 - 2 among them),
    dealt to G lists of 0 .. kin entries, every list ascending by (dist, id).  What follows a list's last entry is
    (+inf, -1) padding or, per `ends`, one of the other three ends of the contract with garbage behind that would win
    if it were read: "nan" (NaN, an id), "inf" (+inf, an id >= 0), "neg" (a small distance, a negative id); "mixed"
    gives most short lists the padding and a few each of the others.  Returns (d [G, kin], i [G, kin])."""
    assert 0 <= M <= G * kin
    slots = np.repeat(np.arange(G), kin)
    owner = np.sort(rng.permutation(slots)[:M])
    dist = rng.choice(values, size=M)
    ids = rng.permutation(3 * M + 8)[:M].astype(np.int64)
    if M:
        ids[rng.integers(M)] = ID_MAX
    order = np.lexsort((ids, dist, owner))  # by list, then (dist, id) within it
    owner, dist, ids = owner[order], dist[order], ids[order]
    lens = np.bincount(owner, minlength=G)
    start = np.concatenate(([0], np.cumsum(lens)[:-1]))
    col = np.arange(M) - start[owner]
    # behind the ends: finite-looking entries below every value of the set but -inf
    d = np.full((G, kin), np.float32(-9e30), dtype=np.float32)
    i = (1000000 + np.arange(G * kin, dtype=np.int64)).reshape(G, kin)
    kind = {"pad": 0, "nan": 1, "inf": 2, "neg": 3}.get(ends, -1)
    e = (np.full(G, kind) if kind >= 0 else rng.choice(4, size=G, p=[0.7, 0.1, 0.1, 0.1]))[:, None]
    at_end = np.arange(kin)[None, :] == lens[:, None]
    behind = (np.arange(kin)[None, :] >= lens[:, None]) & (e == 0)
    d[behind], i[behind] = INF, -1
    d[at_end & (e == 1)] = np.nan
    d[at_end & (e == 2)] = INF
    d[at_end & (e == 3)] = -1e30
    i[at_end & (e == 3)] = -1 - rng.integers(5, size=int(np.sum(at_end & (e == 3))))
    d[owner, col] = dist
    i[owner, col] = ids
    return d, i.astype(np.int32)


def generate(seed, G, kin, fills, values=VALUES, ends="mixed"):
    """fills: the number of entries M of each query; ends: one word for all queries or one per query
    -> (d [G, B, kin], i [G, B, kin])."""
    rng = np.random.default_rng(seed)
    qs = [fill_query(rng, G, kin, int(M), values, ends if isinstance(ends, str) else ends[b]) for b, M in enumerate(fills)]
    return (np.ascontiguousarray(np.stack([q[0] for q in qs], axis=1)),
            np.ascontiguousarray(np.stack([q[1] for q in qs], axis=1)))


# ------------------------------------------------------------------------------------------------ routes
def head_lpt(G, kin):
    """vs_topk_merge_plan's out[0], restated: 0 = compacting kernel, else the list-head kernel's lists per thread."""
    if G * kin <= CAP:
        return 0
    lpt = 1
    while 256 * lpt < G:
        lpt *= 2
    return lpt


def append_order(d, i):
    """The order in which the compacting kernel pools one query's entries (d, i [G, kin]) WHEN G <= 64: then one wave
    owns every list, lane g walks list g, and the lanes of one step append in ascending lane order.  (With more lists
    four waves append side by side and the order is not determined.)  Returns (dists, ids) in that order."""
    G, kin = d.shape
    assert G <= 64
    lens = list_lengths(d, i)
    gs = [g for j in range(kin) for g in range(G) if lens[g] > j]
    js = [j for j in range(kin) for g in range(G) if lens[g] > j]
    return d[gs, js], i[gs, js]


def filter_survivors(cd, ci, kout):
    """The entries the filter sets aside, given a query's pooled entries in append order (more than 256 of them, kout <=
    64): those not above the kout-th smallest of the first 256."""
    assert len(cd) > 256 and kout <= 64
    o = np.lexsort((ci[:256], cd[:256]))[kout - 1]
    td, ti = cd[o], ci[o]
    return int(np.sum((cd < td) | ((cd == td) & (ci <= ti))))


def compact_route(M, kout, S=None):
    """The branch of the compacting kernel that ranks a query of M pooled entries; S = filter_survivors(...) where the
    append order is known, else None."""
    if M > 256 and kout <= 64:
        if S is None:
            return "filter"
        if S <= KEEP:
            return "filter-epl1" if S <= 64 else "filter-epl4" if S <= 256 else "filter-epl16"
        return "overflow-epl16" if M <= 1024 else "overflow-rounds"
    if M <= 64:
        return "epl1"
    if M <= 256:
        return "epl4"
    return "epl16" if M <= 1024 else "rounds"
