"""The IVF index builder at any vector length 1 <= dim <= 2048 (vs_ivf_build_nd, vs_ivf_build_index_nd: the general
k-means++ step, scan_nd_kernel's kModeAssign, the general fixed-point update) against the exact replay of
tests/test_gpu_ivf_build.py, whose helpers are not tied to 128.

Integer data: values in [0, _hi(dim)) with 2 dim (hi - 1)^2 < 2^24 (`_hi` of tests/test_gpu_ivf_nd.py; `_int_norms` asserts
it from the data), a quarter of the rows overwritten by copies of four rows so that real ties exist; the shifted variant
is base - hi // 2 (negative components).  On such rows every quantity is exact in any summation order, so seeds,
assignment and updates are compared bit for bit.  On N(0, 1) rows the assignment is compared with the CPU oracle in the
scan's own summation order ("chain"), for every row, without a tolerance."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle
from test_gpu_ivf_build import (_same_bits, exact_argmin, expected_update_int, kmeans_init, replay_kmeanspp,
                                replay_random_init)
from test_gpu_ivf_nd import _hi

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 20, 100, 130, 384, 960, 2048]
ROWS = [64, 1000, 1025, 3000]
NLISTS = [1, 31, 32, 33, 64, 100]
SEEDS = (0, 42, 2 ** 63 + 12345)
_FORCE_ENV = "VSEARCH_BUILD_ND_FORCE"
VS_OK, VS_ERR_INVALID, VS_ERR_UNSUPPORTED = 0, -1, -5
# the full cross at dim 100; n in {1025, 3000} x nlist in {33, 100} elsewhere
CASES = [(100, n) for n in ROWS] + [(d, n) for d in DIMS if d != 100 for n in (1025, 3000)]


def _nlists(dim, n):
    return [c for c in (NLISTS if dim == 100 else (33, 100)) if c <= n]


@functools.lru_cache(maxsize=4)
def _int_base(dim, n, shifted=False):
    rng = np.random.default_rng(7000 + 31 * dim + n)
    hi = _hi(dim)
    base = rng.integers(0, hi, size=(n, dim)).astype(np.float32)
    q = n // 4
    base[n // 2:n // 2 + q] = base[rng.integers(0, 4, size=q)]
    if shifted:
        base -= hi // 2
    base.setflags(write=False)
    return base


@functools.lru_cache(maxsize=4)
def _gauss_base(dim, n=3000):
    base = np.random.default_rng(8000 + dim).normal(0, 1, size=(n, dim)).astype(np.float32)
    base.setflags(write=False)
    return base


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ------------------------------------------------------------------------------------------------ 1. seeds
@pytest.mark.parametrize("dim,n", CASES)
def test_seeds_equal_the_replay(gpu_pkg, dim, n):
    """max_iter = 0 returns the seeds: base[replayed rows] bit for bit under k-means++ (three seeds) and under
    VSEARCH_KMEANS_INIT=random."""
    base = _int_base(dim, n)
    for nlist in _nlists(dim, n):
        for seed in SEEDS:
            rows = replay_kmeanspp(base, nlist, seed)[0]
            cents, _, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
            assert n_iter == 0 and cents.shape == (nlist, dim)
            assert _same_bits(cents, base[rows]), (dim, n, nlist, seed)
        rows = replay_random_init(n, nlist, 42)
        with kmeans_init("random"):
            cents, _, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, 42)
        assert n_iter == 0 and _same_bits(cents, base[rows]), (dim, n, nlist)


def test_identical_rows_seed_by_the_all_zero_fallback(gpu_pkg):
    base = np.repeat(_int_base(100, 64)[:1], 1500, axis=0)
    nlist = 8
    rows, totals, _ = replay_kmeanspp(base, nlist, 3)
    assert np.all(totals[1:] == 0) and np.all(rows[1:] == len(base) - 1)
    cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, 3)
    assert n_iter == 0 and _same_bits(cents, base[rows]) and np.all(assign == 0)
    full, assign_f, n_iter_f = gpu_pkg.ivf_kmeans(base, nlist, 5, 0.0, 3)
    assert np.all(assign_f == 0) and _same_bits(full, cents) and n_iter_f == 1


def test_fewer_distinct_rows_than_centres(gpu_pkg):
    m, nlist, seed = 5, 9, 11
    distinct = np.ascontiguousarray(_int_base(100, 3000)[[0, 1, 2, 3, 10]])
    assert len(np.unique(distinct, axis=0)) == m
    which = np.random.default_rng(6).integers(0, m, size=2500)
    which[:m] = np.arange(m)
    # three pick blocks (1024 + 1024 + 452 rows): the last row of the base differs from the last row of both earlier
    # blocks and from row 0, so a fallback that lands in another block, or at its start, returns other bits
    which[-1] = 2
    which[[0, 1023, 1024, 2047, 2048]] = [0, 3, 4, 1, 0]
    base = distinct[which]
    rows, totals, _ = replay_kmeanspp(base, nlist, seed)
    assert np.all(totals[1:m] > 0) and np.all(totals[m:] == 0)
    assert len({int(which[r]) for r in rows[:m]}) == m
    assert np.all(rows[m:] == len(base) - 1)
    cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
    assert n_iter == 0 and _same_bits(cents, base[rows])
    want, ties = exact_argmin(base, cents)
    assert ties == int((which == which[-1]).sum()) and np.array_equal(assign, want)
    assert not np.isin(assign, np.arange(m, nlist)).any()
    full, assign_f, n_iter_f = gpu_pkg.ivf_kmeans(base, nlist, 6, 0.0, seed)
    assert _same_bits(full, cents) and np.array_equal(assign_f, want) and n_iter_f == 1


# ------------------------------------------------------------------------------------------------ 2. assignment, integer seeds
@pytest.mark.parametrize("init", ["kmeans++", "random"])
@pytest.mark.parametrize("dim,n", CASES)
def test_assignment_is_the_exact_argmin_with_ties_to_the_lower_id(gpu_pkg, dim, n, init):
    """At max_iter = 0 the centroids are integer rows: the assignment is np.argmin of the exact integer distances for
    every row.  nlist 1 / 31 (remainder launch only), 32 (one full batch), 33 (both launches), 64 (two full batches: the
    kernel must go on to the second), 100 (assign_base > 0)."""
    base = _int_base(dim, n)
    ties_seen = 0
    for nlist in _nlists(dim, n):
        seed = 7 + nlist
        rows = replay_random_init(n, nlist, seed) if init == "random" else replay_kmeanspp(base, nlist, seed)[0]
        with kmeans_init("random" if init == "random" else None):
            cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 0, 0.0, seed)
        assert n_iter == 0 and _same_bits(cents, base[rows]), (dim, n, nlist)
        want, ties = exact_argmin(base, cents)
        bad = np.flatnonzero(assign != want)
        assert bad.size == 0, (dim, n, nlist, init, bad[:5], assign[bad[:5]], want[bad[:5]])
        if nlist > 1:
            ties_seen += ties
    print(f"dim {dim} n {n} {init}: rows with tied nearest centroids over all nlist: {ties_seen}")
    # a condition on the data and the seeds, read from the replayed rows: random initialisation draws the planted block
    # more than once (equal seeds), and at dim 1 the 256 values leave rows midway between two seeds under either init
    if init == "random" or dim == 1:
        assert ties_seen > 0, (dim, n, init)


# ------------------------------------------------------------------------------------------------ 3. assignment, chain oracle
@pytest.mark.parametrize("dim", [20, 130, 960])
def test_assignment_on_non_integer_data_equals_the_chain_oracle(gpu_pkg, dim):
    """N(0, 1) rows, seeds and three updates: the assignment is the first minimum over the centroids of the distance in
    scan_nd_kernel's summation order (oracle dot_order "chain", the reference of
    test_gpu_ivf_nd.py::test_non_integer_data_equals_the_chain_oracle) for EVERY row."""
    base = _gauss_base(dim)
    for t in range(4):
        cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, 33, t, 0.0, 17)
        assert n_iter <= t
        want = np.argmin(oracle.l2_matrix(cents, base, dot_order="chain"), axis=0)
        bad = np.flatnonzero(assign != want)
        assert bad.size == 0, (dim, t, bad[:5], assign[bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------------------------------ 4. update, by induction
_CHAINS = {}
_CHAIN_STEPS = 7
_CHAIN_CASES = {"d20": (20, 3000, 33, 5), "d960": (960, 3000, 33, 11), "d100": (100, 20000, 64, 9)}


def _chain(pkg, name):
    """(centroids, assign, n_iter) of ivf_kmeans(max_iter = t, tol = 0) for t = 0 .. 7 on shifted integer rows."""
    if name not in _CHAINS:
        dim, n, nlist, seed = _CHAIN_CASES[name]
        base = _int_base(dim, n, True)
        _CHAINS[name] = (base, nlist, seed, [pkg.ivf_kmeans(base, nlist, t, 0.0, seed) for t in range(_CHAIN_STEPS + 1)])
    return _CHAINS[name]


@pytest.mark.parametrize("name", list(_CHAIN_CASES))
def test_update_is_the_exact_mean_of_the_previous_assignment(gpu_pkg, name):
    """Induction over t = 0 .. 6: the centroids after t + 1 updates are float32(float64(sum of rows) / count) over the
    assignment the library returned after t updates, empty clusters unchanged."""
    base, nlist, seed, chain = _chain(gpu_pkg, name)
    assert base.min() < 0
    moved = 0
    for t in range(_CHAIN_STEPS):
        prev_c, prev_a, it0 = chain[t]
        next_c, _, it1 = chain[t + 1]
        assert prev_a.min() >= 0 and prev_a.max() < nlist
        want, counts = expected_update_int(base, prev_a, prev_c)
        assert counts.sum() == len(base)
        bad = np.flatnonzero((want.view(np.uint32) != next_c.view(np.uint32)).any(1))
        assert bad.size == 0, (name, t, bad[:5], counts[bad[:5]])
        for c in np.flatnonzero(counts == 0):
            assert _same_bits(next_c[c], prev_c[c])
        assert it0 <= t and it1 <= t + 1
        if not _same_bits(prev_c, next_c):
            assert it1 == t + 1
            moved += 1
    assert moved >= 4
    assert (chain[-1][0] < 0).any()


# ------------------------------------------------------------------------------------------------ 5. update, non-integer rows
def test_update_on_non_integer_data_within_the_fixed_point_bound(gpu_pkg):
    """Per component |centroid - float64 mean over the library's own previous assignment| <= 2^-21 + 2^-24 |mean|: the
    bound derived in test_gpu_ivf_build.py::test_update_on_non_integer_data_within_the_fixed_point_bound (half a
    fixed-point step per row, averaged, plus one cast to fp32); it does not depend on the dimension."""
    base = _gauss_base(130)
    nlist = 33
    b64 = base.astype(np.float64)
    chain = [gpu_pkg.ivf_kmeans(base, nlist, t, 0.0, 17) for t in range(_CHAIN_STEPS + 1)]
    worst = 0.0
    for t in range(_CHAIN_STEPS):
        cents, assign, _ = chain[t]
        nxt = chain[t + 1][0].astype(np.float64)
        counts = np.bincount(assign, minlength=nlist)
        for c in range(nlist):
            if counts[c] == 0:
                assert _same_bits(chain[t + 1][0][c], cents[c])
                continue
            mean = b64[assign == c].sum(0) / counts[c]
            err = np.abs(nxt[c] - mean)
            bound = 2.0 ** -21 + 2.0 ** -24 * np.abs(mean)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (t, c, float(err.max()))
    print(f"dim 130: largest update error / bound {worst:.3f}")
    assert not _same_bits(chain[0][0], chain[_CHAIN_STEPS][0])


# ------------------------------------------------------------------------------------------------ 6. stopping rule
def test_stopping_rule_counts_the_update_that_falls_under_the_tolerance(gpu_pkg):
    """The method of test_gpu_ivf_build.py's test of the same name at dim 100: tolerances at the geometric mean of two
    successive shifts of the exact chain."""
    base, nlist, seed, chain = _chain(gpu_pkg, "d100")
    s = [np.inf] + [float(((chain[t][0].astype(np.float64) - chain[t - 1][0].astype(np.float64)) ** 2).sum())
                    for t in range(1, _CHAIN_STEPS + 1)]
    mv = float(base.astype(np.float64).var(axis=0).mean())
    print(f"d100: shifts {['%.4g' % v for v in s[1:]]}, mean feature variance {mv:.6g}")
    js = [j for j in range(1, _CHAIN_STEPS)
          if s[j] > 1.05 * s[j + 1] and s[j + 1] > 0 and min(s[1:j + 1]) > np.sqrt(s[j] * s[j + 1])]
    assert len(js) >= 2, s  # the replayed shifts must offer two stopping points
    for j in (js[0], js[-1]):
        tol = np.sqrt(s[j] * s[j + 1]) / mv
        cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, 50, tol, seed)
        assert n_iter == j + 1, (j, n_iter, s)
        assert _same_bits(cents, chain[j + 1][0]) and np.array_equal(assign, chain[j + 1][1])
    j = js[-1]  # a max_iter below the stopping point wins
    cents, _, n_iter = gpu_pkg.ivf_kmeans(base, nlist, j, np.sqrt(s[j] * s[j + 1]) / mv, seed)
    assert n_iter == j and _same_bits(cents, chain[j][0])


def test_zero_tolerance_stops_at_the_first_update_that_moves_nothing(gpu_pkg):
    base = _int_base(100, 1000, True)[:600]
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


# ------------------------------------------------------------------------------------------------ 7. dim 128 and the toggle
def _raw_nd(pkg, base, nlist, max_iter=3, tol=0.0, dim=None, seed=1, sentinel=False):
    """vs_ivf_build_nd through ctypes: (status, centroids, assign, n_iter); the outputs start sentinel filled."""
    base = np.ascontiguousarray(base, dtype=np.float32)
    n, d = base.shape
    cents = np.full((nlist, d), -7.25, dtype=np.float32)
    assign = np.full(n, -77, dtype=np.int32)
    it = C.c_int(-55)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().vs_ivf_build_nd(p(base), n, d if dim is None else dim, nlist, max_iter, tol, seed, 0, p(cents), p(assign),
                                   C.byref(it))
    if sentinel:
        untouched = bool(np.all(cents == -7.25) and np.all(assign == -77) and it.value == -55)
        return rc, pkg.lib().vs_last_error().decode(), untouched
    return rc, cents, assign, it.value


@pytest.mark.parametrize("shift", [0.0, 128.0])
def test_dim_128_equals_vs_ivf_build_with_and_without_the_toggle(gpu_pkg, shift):
    base = gpu_pkg.synth_sift(3000, seed=51) - np.float32(shift)
    for nlist in (33, 100):
        for max_iter in (0, 3):
            cents, assign, n_iter = gpu_pkg.ivf_kmeans(base, nlist, max_iter, 0.0, 42)  # vs_ivf_build
            for force in (None, "1"):
                with _env(_FORCE_ENV, force):
                    rc, c2, a2, it2 = _raw_nd(gpu_pkg, base, nlist, max_iter, 0.0, seed=42)
                assert rc == VS_OK and it2 == n_iter, (nlist, max_iter, force, it2, n_iter)
                assert _same_bits(c2, cents), (nlist, max_iter, force)
                assert np.array_equal(a2, assign), (nlist, max_iter, force)
    assert os.environ.get(_FORCE_ENV) is None


# ------------------------------------------------------------------------------------------------ 8. end to end
@pytest.mark.parametrize("dim", [100, 384])
def test_build_index_end_to_end(gpu_pkg, dim, tmp_path):
    n, nlist, max_iter, seed = 6000, 24, 5, 42
    rng = np.random.default_rng(8800 + dim)
    hi = _hi(dim)
    base = rng.integers(0, hi, size=(n, dim)).astype(np.float32)
    q = rng.integers(0, hi, size=(70, dim)).astype(np.float32)
    vr, off, r2o, cents, n_iter = gpu_pkg.ivf_build(base, nlist, max_iter, 0.0, seed)
    assert cents.shape == (nlist, dim) and off[-1] == n
    ivf, n_iter_b = gpu_pkg.IVFIndex.build(base, nlist, max_iter, 0.0, seed)
    with ivf:
        assert n_iter_b == n_iter
        assert ivf.getDim() == dim and ivf.getNumVectors() == n and ivf.getNumClusters() == nlist
        want = {}
        for k, nprobe in ((1, 1), (5, 4), (16, nlist)):
            oi, od, ototal = oracle.ivf_search(vr, off, r2o, cents, q, k, nprobe, dot_order="chain")
            ids, d, total = ivf.searchBatch(q, len(q), k, nprobe)
            assert np.array_equal(ids, oi) and np.array_equal(d.view(np.int32), od.view(np.int32)) and total == ototal, (dim, k, nprobe)
            want[(k, nprobe)] = (oi, od, ototal)
        ivf.save(str(tmp_path / "idx"))
    with gpu_pkg.IVFIndex(str(tmp_path / "idx")) as again:
        assert again.getDim() == dim
        for (k, nprobe), (oi, od, ototal) in want.items():
            ids, d, total = again.searchBatch(q, len(q), k, nprobe)
            assert np.array_equal(ids, oi) and np.array_equal(d.view(np.int32), od.view(np.int32)) and total == ototal, (dim, k, nprobe)
    # nprobe = nlist scans every row: the exact answer.  Equal distances would rank by reordered position here and by id
    # there; the data has none among a query's best 16 (a condition on the data)
    oi, od, _ = want[(16, nlist)]
    assert (np.diff(od, axis=1) > 0).all()
    with gpu_pkg.BruteForceIndex(base) as bf:  # (a general brute-force index takes k <= 15)
        bf_ids, bf_d = bf.search(q, 15)
    assert np.array_equal(bf_ids, oi[:, :15]) and np.array_equal(bf_d.view(np.int32), od[:, :15].view(np.int32))


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_outputs_alone(gpu_pkg):
    good = _int_base(100, 1000)
    for bad_value in (np.nan, np.inf, -np.inf):
        for tol in (0.0, 1e-4):
            base = good.copy()
            base[999, 99] = bad_value
            rc, msg, untouched = _raw_nd(gpu_pkg, base, 8, tol=tol, sentinel=True)
            assert rc == VS_ERR_INVALID and msg and untouched, (bad_value, tol, rc, msg)
    big = good.copy()
    big[517, 3] = -2.0 ** 34                                    # 1000 * 2^34 > 2^43
    rc, msg, untouched = _raw_nd(gpu_pkg, big, 8, sentinel=True)
    assert rc == VS_ERR_INVALID and "2^43" in msg and untouched
    rc, msg, untouched = _raw_nd(gpu_pkg, good, 8, dim=0, sentinel=True)
    assert rc == VS_ERR_INVALID and untouched
    rc, msg, untouched = _raw_nd(gpu_pkg, good, 8, dim=2049, sentinel=True)
    assert rc == VS_ERR_UNSUPPORTED and "2048" in msg and untouched
    rc, msg, untouched = _raw_nd(gpu_pkg, good, 1001, sentinel=True)   # nlist > n_rows
    assert rc == VS_ERR_INVALID and untouched
    rc, msg, untouched = _raw_nd(gpu_pkg, good, 8, max_iter=-1, sentinel=True)
    assert rc == VS_ERR_INVALID and untouched
    rc, cents, assign, n_iter = _raw_nd(gpu_pkg, good, 8)       # a good call afterwards still works
    assert rc == VS_OK and n_iter >= 1 and assign.min() >= 0 and assign.max() < 8
    assert np.array_equal(assign, np.argmin(oracle.l2_matrix(cents, good, dot_order="chain"), axis=0))
