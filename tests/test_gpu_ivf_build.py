"""The IVF index builder (vs_ivf_build: k-means++ seeding, kModeAssign, the fixed-point Lloyd update, the stopping
rule) against an exact replay on the CPU.

On integer-valued rows every quantity the builder computes is exact and independent of the order in which threads
arrive: squared distances are integers below 2^24, their double sums are exact, the 44.20 fixed-point cluster sums are
exact, and float(double(sum) / count) is one division and one cast that numpy repeats.  So seeds, assignment and every
update are compared bit for bit.  The stream, the pick rule, the tie rule, the empty-cluster rule and the meaning of
n_iter that the replay uses are the ones include/vsearch.h states at vs_ivf_build."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

_M64 = (1 << 64) - 1
_INIT_ENV = "VSEARCH_KMEANS_INIT"
VS_OK, VS_ERR_INVALID = 0, -1  # vs_status (include/vsearch.h)


# ------------------------------------------------------------------------------------------------ the replay
class SplitMix64:
    """The builder's seeding stream (vsearch.h): state seed * 0x9E3779B97F4A7C15 + 0x1234567, then splitmix64."""

    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & _M64

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def unit(self):
        return float(self.next() >> 11) * 2.0 ** -53  # both factors exact


def _int_norms(base):
    """Exact squared norms of integer-valued fp32 rows, and the check that the card's fp32 distances are exact too:
    ||x||^2 + ||c||^2 and every distance stay below 2^24."""
    assert np.array_equal(base, np.rint(base))
    bn = np.einsum("ij,ij->i", base, base)  # fp32 sums of integers below 2^24: exact in any order
    top = float(bn.max())
    assert 2 * top < 2 ** 24 and (base.min() >= 0 or 4 * top < 2 ** 24)
    return bn.astype(np.float64)


def _d2_to(base, bn, c):
    """Exact squared distances of all rows to the integer row c.  The fp32 product is exact: every partial sum is an
    integer of magnitude <= ||x|| ||c|| < 2^23."""
    return bn + float((c.astype(np.float64) ** 2).sum()) - 2.0 * (base @ c).astype(np.float64)


def replay_kmeanspp(base, nlist, seed):
    """Rows the builder seeds with: first next() % n, then for every further centre the first row whose running D^2
    sum exceeds u * total (the last row when every D^2 is zero).  Returns (rows, totals, final D^2); totals[c] is the
    D^2 sum centre c was drawn from (totals[0] = inf)."""
    n = len(base)
    bn = _int_norms(base)
    rng = SplitMix64(seed)
    rows = [rng.next() % n]
    totals = [np.inf]
    d2 = np.full(n, np.inf)
    for _ in range(1, nlist):
        d2 = np.minimum(d2, _d2_to(base, bn, base[rows[-1]]))
        cum = np.cumsum(d2)  # integers below 2^53: exact
        u = rng.unit()
        pick = int(np.searchsorted(cum, u * cum[-1], side="right"))
        rows.append(min(pick, n - 1))
        totals.append(float(cum[-1]))
    d2 = np.minimum(d2, _d2_to(base, bn, base[rows[-1]]))
    return np.array(rows), np.array(totals), d2


def replay_random_init(n, nlist, seed):
    """VSEARCH_KMEANS_INIT=random: next() % n, drawn again while the row number is taken."""
    rng = SplitMix64(seed)
    used, rows = set(), []
    for _ in range(nlist):
        r = rng.next() % n
        while r in used:
            r = rng.next() % n
        used.add(r)
        rows.append(r)
    return np.array(rows)


def exact_argmin(base, cents, chunk=4096):
    """Nearest integer centroid of every integer row by exact integer distances, lowest id among equals (np.argmin
    returns the first minimum); also the number of rows whose minimum is shared by several centroids."""
    out = np.empty(len(base), dtype=np.int64)
    ties = 0
    for r0 in range(0, len(base), chunk):
        ex = oracle.exact_int_dists(base[r0:r0 + chunk], cents)
        out[r0:r0 + chunk] = ex.argmin(1)
        ties += int(((ex == ex.min(1, keepdims=True)).sum(1) > 1).sum())
    return out, ties


def expected_update_int(base, assign, prev_cents):
    """One Lloyd update on integer-valued rows: float32(float64(sum of rows) / count); a cluster without rows keeps
    its centroid."""
    bi = base.astype(np.int64)
    out = prev_cents.copy()
    counts = np.bincount(assign, minlength=len(prev_cents))
    for c in np.flatnonzero(counts):
        s = bi[assign == c].sum(0)
        assert np.abs(s).max() < 2 ** 53
        out[c] = (s.astype(np.float64) / float(counts[c])).astype(np.float32)
    return out, counts


@contextlib.contextmanager
def kmeans_init(value):
    old = os.environ.get(_INIT_ENV)
    try:
        if value is None:
            os.environ.pop(_INIT_ENV, None)
        else:
            os.environ[_INIT_ENV] = value
        yield
    finally:
        if old is None:
            os.environ.pop(_INIT_ENV, None)
        else:
            os.environ[_INIT_ENV] = old


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ a. seeds
_NLISTS = (1, 2, 31, 32, 33, 64, 100)


@pytest.mark.parametrize("n", [64, 1000, 1024, 1025, 3000, 30000])
def test_seeds_equal_the_replay(gpu_pkg, n):
    """max_iter = 0 returns the k-means++ seeds: base[replayed rows] bit for bit, for row counts around one pick block
    (1024 rows) and several of them, nlist around the 32-centroid scan block, three seeds each."""
    base = gpu_pkg.synth_sift(n, seed=100 + n)
    checked = 0
    for nlist in _NLISTS:
        if nlist > n:
            continue
        for seed in (0, 42, 2 ** 63 + 12345):
            rows, totals, d2 = replay_kmeanspp(base, nlist, seed)
            # the fast replay distances are the oracle's exact integers
            assert np.array_equal(d2, oracle.exact_int_dists(base[rows], base).min(0))
            cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
            assert n_iter == 0
            assert _same_bits(cents, base[rows]), (n, nlist, seed)
            # D^2 sampling never draws a row at distance 0 from an earlier seed while another row is left
            for c in range(1, nlist):
                if totals[c] > 0:
                    assert np.abs(cents[:c] - cents[c]).max(1).min() > 0, (n, nlist, seed, c)
            checked += 1
    assert checked >= 15


# ------------------------------------------------------------------------------------------------ b. > 1024 pick blocks
def _two_chunk_base(pkg):
    """1 100 000 rows = 1075 pick blocks, 51 past the first 1024-block chunk of kpp_pick_kernel.  Rows from 1 048 576 on
    are an outlying group: uniform integers in [0, 218], far from the clustered rows and from each other, so that D^2
    sampling keeps drawing from them."""
    n, cut = 1_100_000, 1_048_576
    base = np.empty((n, 128), dtype=np.float32)
    base[:cut] = pkg.synth_sift(cut, seed=77)
    base[cut:] = np.random.default_rng(77).integers(0, 219, size=(n - cut, 128)).astype(np.float32)
    return base, cut


def test_seeds_beyond_1024_pick_blocks(gpu_pkg):
    base, cut = _two_chunk_base(gpu_pkg)
    nlist, seed = 64, 42
    rows, totals, d2 = replay_kmeanspp(base, nlist, seed)
    # condition on the data, from the replay alone: the second chunk of block sums is really walked
    assert int((rows >= cut).sum()) >= 3, rows
    assert int((rows < cut).sum()) >= 3, rows
    probe = np.r_[0:len(base):257, cut - 2000:cut + 2000, len(base) - 2000:len(base)]
    assert np.array_equal(d2[probe], oracle.exact_int_dists(base[rows], base[probe]).min(0))
    cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
    assert n_iter == 0
    first_bad = np.flatnonzero((cents != base[rows]).any(1))
    assert _same_bits(cents, base[rows]), f"first differing seed {first_bad[:1]}, replayed rows {rows}"
    for c in range(1, nlist):
        assert np.abs(cents[:c] - cents[c]).max(1).min() > 0
    # the assignment of 1.1 M rows to the integer seeds: spot-checked exactly
    want, _ = exact_argmin(base[probe], cents)
    assert np.array_equal(assign[probe], want)


# ------------------------------------------------------------------------------------------------ c. degenerate seeding
def test_identical_rows_seed_by_the_all_zero_fallback(gpu_pkg):
    row = gpu_pkg.synth_sift(1, seed=5)
    base = np.repeat(row, 1500, axis=0)
    nlist = 8
    rows, totals, _ = replay_kmeanspp(base, nlist, 3)
    assert np.all(totals[1:] == 0) and np.all(rows[1:] == len(base) - 1)
    cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, 3)
    assert n_iter == 0 and _same_bits(cents, base[rows]) and np.all(assign == 0)
    full, assign_f, n_iter_f = gpu_pkg.ivf_kmeans(base, nlist, 5, 0.0, 3)
    # every row ties between all eight centroids and goes to id 0; clusters 1..7 stay empty and keep their centroid
    assert np.all(assign_f == 0) and _same_bits(full, cents) and n_iter_f == 1


def test_fewer_distinct_rows_than_centres(gpu_pkg):
    m, nlist, seed = 5, 9, 11
    distinct = gpu_pkg.synth_sift(m, seed=6)
    which = np.random.default_rng(6).integers(0, m, size=2500)
    which[:m] = np.arange(m)
    # three pick blocks (1024 + 1024 + 452 rows): the last row of the base differs from the last row of both earlier
    # blocks and from row 0, so a fallback that lands in another block, or at its start, returns other bits
    which[-1] = 2
    which[[0, 1023, 1024, 2047, 2048]] = [0, 3, 4, 1, 0]
    base = distinct[which]
    assert len(np.unique(base, axis=0)) == m
    rows, totals, _ = replay_kmeanspp(base, nlist, seed)
    assert np.all(totals[1:m] > 0) and np.all(totals[m:] == 0)
    assert len({int(which[r]) for r in rows[:m]}) == m          # the first m seeds are the m distinct rows
    assert np.all(rows[m:] == len(base) - 1)                     # the rest: the fallback
    cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
    assert n_iter == 0 and _same_bits(cents, base[rows])
    want, ties = exact_argmin(base, cents)
    assert ties == int((which == which[-1]).sum()) and np.array_equal(assign, want)
    assert not np.isin(assign, np.arange(m, nlist)).any()        # the duplicates lose every tie to the lower id
    full, assign_f, n_iter_f = gpu_pkg.ivf_kmeans(base, nlist, 6, 0.0, seed)
    # means of identical rows are those rows: nothing moves, the duplicate clusters stay empty and unchanged
    assert _same_bits(full, cents) and np.array_equal(assign_f, want) and n_iter_f == 1
    for c in range(m, nlist):
        assert not (assign_f == c).any() and _same_bits(full[c], cents[c])


# ------------------------------------------------------------------------------------------------ d. random init
@pytest.mark.parametrize("n,nlist", [(64, 64), (1000, 33), (3000, 1500), (30000, 100)])
def test_random_init_equals_the_rejection_loop(gpu_pkg, n, nlist):
    """n = nlist = 64 and 1500 of 3000 force many rejected draws."""
    base = gpu_pkg.synth_sift(n, seed=200 + n)
    for seed in (1, 42):
        rows = replay_random_init(n, nlist, seed)
        assert len(set(rows.tolist())) == nlist
        with kmeans_init("random"):
            cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
        assert n_iter == 0 and _same_bits(cents, base[rows])
    assert os.environ.get(_INIT_ENV) != "random"
    # and without the variable the same call seeds by k-means++
    if nlist < n:
        cents_pp, _, _ = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, 42)
        assert _same_bits(cents_pp, base[replay_kmeanspp(base, nlist, 42)[0]])


# ------------------------------------------------------------------------------------------------ e. assignment
def _assign_case(pkg, n):
    """SIFT-shaped rows with a quarter of them overwritten by copies of four rows: random initialisation then usually
    draws equal seeds (about nlist / 4 draws from four values), and every row equal to those has a real tie.  Whether it
    did is read from the replayed rows in the test."""
    base = pkg.synth_sift(n, seed=300 + n)
    q = n // 4
    base[n // 2:n // 2 + q] = base[np.random.default_rng(n).integers(0, 4, size=q)]
    return base


@pytest.mark.parametrize("init", ["kmeans++", "random"])
@pytest.mark.parametrize("n", [1000, 4099, 30000])
def test_assignment_is_the_exact_argmin_with_ties_to_the_lower_id(gpu_pkg, n, init):
    """At max_iter = 0 the centroids are integer rows: the assignment must be np.argmin of the exact integer distances
    for every row.  nlist 31 / 32 / 33 / 64 / 100 / 1500: one remainder launch, full blocks only, both, assign_base > 0."""
    base = _assign_case(gpu_pkg, n)
    ties_seen = coinciding = 0
    for nlist in (1, 31, 32, 33, 64, 100, 1500):
        if nlist > n:
            continue
        seed = 7 + nlist
        if init == "random":
            rows = replay_random_init(n, nlist, seed)
        else:
            rows = replay_kmeanspp(base, nlist, seed)[0]
        with kmeans_init("random" if init == "random" else None):
            cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
        assert n_iter == 0 and _same_bits(cents, base[rows]), (n, nlist)
        want, ties = exact_argmin(base, cents)
        bad = np.flatnonzero(assign != want)
        assert bad.size == 0, (n, nlist, init, bad[:5], assign[bad[:5]], want[bad[:5]])
        # seeds that coincide (from the replayed rows alone): every row equal to such a seed is at distance 0 from
        # several centroids, a real tie
        vals, first, cnt = np.unique(base[rows], axis=0, return_index=True, return_counts=True)
        if (cnt > 1).any():
            tied_rows = sum(int((base == v).all(1).sum()) for v in vals[cnt > 1])
            assert ties >= tied_rows > 0, (n, nlist, ties, tied_rows)
            coinciding += 1
        ties_seen += ties
    print(f"n {n} {init}: rows with tied nearest centroids over all nlist: {ties_seen}, nlist values with equal seeds: {coinciding}")
    if init == "random":
        assert coinciding >= 3  # a condition on the data and the seeds, not on the library: the planted block is drawn twice


# ------------------------------------------------------------------------------------------------ f. update, by induction
_CHAINS = {}
_CHAIN_STEPS = 7


def _chain_data(pkg, name):
    if name == "sift-128":     # negative components: the two's-complement path of the unsigned atomics
        return pkg.synth_sift(30000, seed=21) - 128.0, 100, 42
    if name == "sift-odd":     # 4099 rows: less than one grid stride of the accumulation kernel, nlist one past a block
        return pkg.synth_sift(4099, seed=22), 33, 5
    if name == "weak":         # weakly clustered: many rows change cluster at every step
        return pkg.synth_mixture(20000, seed=23, **pkg.WEAK_MIXTURE) - 100.0, 64, 9
    raise KeyError(name)


def _chain(pkg, name):
    """(centroids, assign, n_iter) of ivf_kmeans(max_iter = t, tol = 0) for t = 0 .. 7."""
    if name not in _CHAINS:
        base, nlist, seed = _chain_data(pkg, name)
        _CHAINS[name] = (base, nlist, seed, [pkg.ivf_kmeans(base, nlist, t, 0.0, seed) for t in range(_CHAIN_STEPS + 1)])
    return _CHAINS[name]


@pytest.mark.parametrize("name", ["sift-128", "sift-odd", "weak"])
def test_update_is_the_exact_mean_of_the_previous_assignment(gpu_pkg, name):
    """Induction over t = 0 .. 6: the centroids after t + 1 updates are float32(float64(sum of rows) / count) over the
    assignment the library returned after t updates (which is the assignment to those centroids), empty clusters
    unchanged.  Each step is compared with the library's own previous state, so near-tie divergence cannot
    accumulate, while any wrong sum, count, sign or stride shows."""
    base, nlist, seed, chain = _chain(gpu_pkg, name)
    moved = 0
    for t in range(_CHAIN_STEPS):
        prev_c, prev_a, it0 = chain[t]
        next_c, _, it1 = chain[t + 1]
        assert prev_a.min() >= 0 and prev_a.max() < nlist
        want, counts = expected_update_int(base, prev_a, prev_c)
        assert counts.sum() == len(base)
        bad = np.flatnonzero((want.view(np.uint32) != next_c.view(np.uint32)).any(1))
        assert bad.size == 0, (name, t, bad[:5], counts[bad[:5]])
        assert it0 <= t and it1 <= t + 1
        if not _same_bits(prev_c, next_c):
            assert it1 == t + 1  # tol = 0: no stop before an update moves nothing
            moved += 1
    assert moved >= 4  # the chain is not a fixed point from the start
    if name == "sift-128":
        assert base.min() < 0 and (chain[-1][0] < 0).any()


# ------------------------------------------------------------------------------------------------ g. non-integer data
@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e3])
def test_update_on_non_integer_data_within_the_fixed_point_bound(gpu_pkg, scale):
    """Update: a row enters its cluster sum as rint(x * 2^20) * 2^-20, off by at most half a fixed-point step, 2^-21; the
    sum of those integers is exact, so the mean of the quantised rows is off by at most 2^-21 from the mean of the rows
    (an average of errors that are each at most 2^-21).  The division is done in double (relative 2^-53, nothing
    here) and the result is cast to fp32 once: at most half an ulp, 2^-24 |mean|.  Bound per component:
    2^-21 + 2^-24 |mean|, against the float64 mean over the assignment the library itself returned.

    Assignment: checked separately against the float64 argmin.  With S = max ||c||^2 + max ||x||^2, u = 2^-24,
    gamma = 128 u / (1 - 128 u): two fp32 summation orders of a 128-term dot product differ by at most
    2 gamma ||c|| ||x|| <= gamma S, the epilogue doubles that and adds at most 4 u S of its own (the bound of
    test_gpu_nd.py::test_non_integer_data_within_derived_tolerance at dim 128): tol = (2 gamma + 4 u) S.  Both the
    chosen and the best centroid's fp32 distance carry that error, so chosen - best <= 2 tol in exact arithmetic."""
    rng = np.random.default_rng(900)
    base = (rng.normal(0, 1, size=(20000, 128)) * scale).astype(np.float32)
    nlist, seed = 64, 17
    b64 = base.astype(np.float64)
    bn = (b64 ** 2).sum(1)
    u = 2.0 ** -24
    gamma = 128 * u / (1 - 128 * u)
    chain = [gpu_pkg.ivf_kmeans(base, nlist, t, 0.0, seed) for t in range(_CHAIN_STEPS + 1)]
    worst_ratio, worst_err, worst_bound, worst_gap, worst_tol = 0.0, 0.0, 0.0, 0.0, 0.0
    for t in range(_CHAIN_STEPS + 1):
        cents, assign, _ = chain[t]
        c64 = cents.astype(np.float64)
        cn = (c64 ** 2).sum(1)
        d = bn[:, None] + cn[None, :] - 2.0 * (b64 @ c64.T)
        tol = (2 * gamma + 4 * u) * float(cn.max() + bn.max())
        gap = d[np.arange(len(base)), assign] - d.min(1)
        worst_gap, worst_tol = max(worst_gap, float(gap.max())), max(worst_tol, tol)
        assert gap.max() <= 2 * tol, (scale, t, float(gap.max()), tol)
        if t == _CHAIN_STEPS:
            break
        nxt = chain[t + 1][0].astype(np.float64)
        counts = np.bincount(assign, minlength=nlist)
        for c in range(nlist):
            if counts[c] == 0:
                assert _same_bits(chain[t + 1][0][c], cents[c])
                continue
            mean = b64[assign == c].sum(0) / counts[c]
            err = np.abs(nxt[c] - mean)
            bound = 2.0 ** -21 + 2.0 ** -24 * np.abs(mean)
            i = int(np.argmax(err / bound))
            if err[i] / bound[i] > worst_ratio:
                worst_ratio, worst_err, worst_bound = float(err[i] / bound[i]), float(err[i]), float(bound[i])
            assert np.all(err <= bound), (scale, t, c, float(err[i]), float(bound[i]))
    print(f"scale {scale:g}: largest update error / bound {worst_ratio:.3f} (error {worst_err:.3e}, bound {worst_bound:.3e}); "
          f"largest chosen - best {worst_gap:.3e} against 2 tol {2 * worst_tol:.3e}")
    assert not _same_bits(chain[0][0], chain[_CHAIN_STEPS][0])


# ------------------------------------------------------------------------------------------------ h. stopping rule
def _mean_feature_variance(base):
    return float(base.astype(np.float64).var(axis=0).mean())


@pytest.mark.parametrize("name", ["sift-128", "weak"])
def test_stopping_rule_counts_the_update_that_falls_under_the_tolerance(gpu_pkg, name):
    """s_t = sum of squared centroid shifts of update t (t = 1 .. 7, from the chain of exact updates above), tol_abs =
    tol * mean per-feature variance.  With tol_abs the geometric mean of s_j > s_(j+1), and every earlier shift above
    it, the build performs j + 1 updates: n_iter = j + 1 and the centroids are the chain's after j + 1 updates.  The
    margin is a factor sqrt(s_j / s_(j+1)) > sqrt(1.05), far above the kernel's fp32 reduction error (about 128 * 2^-24 relative)."""
    base, nlist, seed, chain = _chain(gpu_pkg, name)
    s = [np.inf] + [float(((chain[t][0].astype(np.float64) - chain[t - 1][0].astype(np.float64)) ** 2).sum())
                    for t in range(1, _CHAIN_STEPS + 1)]
    mv = _mean_feature_variance(base)
    print(f"{name}: shifts {['%.4g' % v for v in s[1:]]}, mean feature variance {mv:.6g}")
    js = [j for j in range(1, _CHAIN_STEPS)
          if s[j] > 1.05 * s[j + 1] and s[j + 1] > 0 and min(s[1:j + 1]) > np.sqrt(s[j] * s[j + 1])]
    assert len(js) >= 2, s  # the replayed shifts must offer two stopping points
    for j in (js[0], js[-1]):
        tol = np.sqrt(s[j] * s[j + 1]) / mv
        cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 50, tol, seed)
        assert n_iter == j + 1, (name, j, n_iter, s)
        assert _same_bits(cents, chain[j + 1][0]) and np.array_equal(assign, chain[j + 1][1])
    # a max_iter below the stopping point wins
    j = js[-1]
    cents, _, n_iter = gpu_pkg.ivf_kmeans(base, nlist, j, np.sqrt(s[j] * s[j + 1]) / mv, seed)
    assert n_iter == j and _same_bits(cents, chain[j][0])


def test_zero_tolerance_stops_at_the_first_update_that_moves_nothing(gpu_pkg):
    base = gpu_pkg.synth_sift(600, seed=31) - 128.0
    nlist, seed = 4, 2
    cents, assign, T = gpu_pkg.ivf_kmeans(base, nlist, 500, 0.0, seed)
    assert 2 <= T < 500
    at = {t: gpu_pkg.ivf_kmeans(base, nlist, t, 0.0, seed) for t in (T - 2, T - 1, T, T + 7)}
    assert [at[t][2] for t in (T - 2, T - 1, T, T + 7)] == [T - 2, T - 1, T, T]
    assert not _same_bits(at[T - 2][0], at[T - 1][0])   # update T - 1 still moved a centroid
    assert _same_bits(at[T - 1][0], at[T][0])           # update T is the first that moves nothing
    assert _same_bits(at[T + 7][0], at[T][0]) and _same_bits(cents, at[T][0])
    assert np.array_equal(at[T + 7][1], at[T][1]) and np.array_equal(assign, at[T][1])
    want, _ = expected_update_int(base, at[T][1], at[T][0])
    assert _same_bits(want, at[T][0])                   # a fixed point of the exact update


# ------------------------------------------------------------------------------------------------ i. refusals
def _raw_build(pkg, base, nlist, max_iter=3, tol=0.0, dim=None):
    """vs_ivf_build through ctypes with sentinel-filled outputs: (status, error text, outputs untouched)."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    n, d = base.shape
    cents = np.full((nlist, d), -7.25, dtype=np.float32)
    assign = np.full(n, -77, dtype=np.int32)
    it = C.c_int(-55)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().vs_ivf_build(p(base), n, d if dim is None else dim, nlist, max_iter, tol, 1, 0, p(cents), p(assign), C.byref(it))
    untouched = bool(np.all(cents == -7.25) and np.all(assign == -77) and it.value == -55)
    return rc, pkg.lib().vs_last_error().decode(), untouched


def _limit_base(top):
    """1024 integer-valued rows of large magnitude, both signs, with max |x| = top exactly: n_rows * max|x| = 1024 top."""
    rng = np.random.default_rng(41)
    base = np.rint(rng.uniform(-0.9, 0.9, size=(1024, 128)) * top).astype(np.float32)
    base[517, 3] = -top
    assert np.abs(base).max() == top
    return base


def test_refusals_leave_the_outputs_alone(gpu_pkg):
    good = gpu_pkg.synth_sift(1024, seed=40)
    for bad_value in (np.nan, np.inf, -np.inf):
        for tol in (0.0, 1e-4):
            base = good.copy()
            base[1000, 127] = bad_value
            rc, msg, untouched = _raw_build(gpu_pkg, base, 8, tol=tol)
            assert rc == VS_ERR_INVALID and msg and untouched, (bad_value, tol, rc, msg)
    rc, msg, untouched = _raw_build(gpu_pkg, _limit_base(2.0 ** 33), 8)   # 1024 * 2^33 = 2^43
    assert rc == VS_ERR_INVALID and "2^43" in msg and untouched
    rc, msg, untouched = _raw_build(gpu_pkg, _limit_base(2.0 ** 40), 8, tol=1e-4)
    assert rc == VS_ERR_INVALID and msg and untouched
    rc, msg, untouched = _raw_build(gpu_pkg, good, 8)
    assert rc == VS_OK and not untouched


def test_a_base_just_inside_the_magnitude_limit_builds_exactly(gpu_pkg):
    """max |x| = 2^33 - 2^10 (the fp32 number below 2^33), 1024 rows: n_rows * max|x| = 2^43 - 2^20.  The cluster sums
    reach the top bits of the 64-bit accumulators and must still be exact."""
    top = 2.0 ** 33 - 2.0 ** 10
    assert np.float32(top) == top
    base = _limit_base(top)
    base[:300] = np.float32(top)   # 300 rows of +top in every column: one cluster's sums near 300 * 2^53
    base[300:600] = np.float32(-top)
    nlist, seed = 8, 4
    chain = [gpu_pkg.ivf_kmeans(base, nlist, t, 0.0, seed) for t in range(4)]
    assert np.abs(chain[0][0]).max() == top
    for t in range(3):
        want, counts = expected_update_int(base, chain[t][1], chain[t][0])
        assert _same_bits(want, chain[t + 1][0]), (t, counts)
    assert counts.max() >= 300
