"""The single-call scan of a general index (scan_one_nd_kernel): short device calls -- fewer than 4 batches of
at most 16 queries, k <= 15 -- on the fp32 rows of a vs_bf_create_nd index are ONE launch per batch.

Every case asserts first, through vs_bf_one_plan with the device's CU count, that its call is on route 2: on a library
without the kernel the symbol is missing and every test fails.  Expected values: the CPU oracle on integer data (exact in
any order), the chain oracle's bits on real-valued data where distances cancel (tests/cancel_data.py), the float64
product under inner product -- the references of test_gpu_nd.py, test_gpu_cancel.py and test_gpu_ip.py, imported."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import cancel_data  # noqa: E402
import nd_one_child  # noqa: E402
import oracle  # noqa: E402
import test_gpu_cancel as tc  # noqa: E402
import test_gpu_ip as tip  # noqa: E402
from cancel_data import bits  # noqa: E402
from test_gpu_nd import _int_data  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (("one", 1, 1), ("one", 1, 7), ("one", 1, 16), ("multi", 3, 16))  # (call, batches, queries per batch)
KS = (1, 5, 15)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _on_route_2(pkg, n, dim, nb, B, k):
    plan = pkg.BruteForceIndex.one_plan(n, dim, _cus(), nb, B, k)
    assert plan[0] == 2, (n, dim, nb, B, k, plan)
    return plan


def _tie_flags(d):
    return (d[:, 1:] == d[:, :-1]).any(1)


def _sorted_int_ref(base, q, k1, id_offset=0):
    """the k1 best by (distance, id) from the oracle's exact distances, (-1, +inf) past the rows"""
    n = len(base)
    ids = np.full((len(q), k1), -1, dtype=np.int32)
    d = np.full((len(q), k1), np.inf, dtype=np.float32)
    for i in range(len(q)):
        row = oracle.l2_row(q[i], base)
        o = np.lexsort((np.arange(n), row))[:k1]
        ids[i, :len(o)] = o + id_offset
        d[i, :len(o)] = row[o]
    return ids, d


def _check_int(got, oi, od, sref, tag):
    """Distances of every query and flags = two equal distances among the k + 1, against oracle.search_bf's (oi, od).
    Ids against it where the flag is 0 -- except the last id of a query whose (k + 1)-th and (k + 2)-th best are equal
    (integer distances of 20 000 rows repeat often, and _int_data draws the sources of its copies with replacement): no
    flag can tell, select_topk keeps whichever it met first, the kernel the lower id.  What the kernel promises covers those too and is asserted for EVERY query:
    the k + 1 best by (distance, id), from sref = _sorted_int_ref(.., at least k + 2)."""
    gi, gd, fl = got
    n, k1 = gd.shape
    si, sd = sref[0][:n], sref[1][:n]
    assert np.array_equal(gd, od), (tag, "distances", np.nonzero((gd != od).any(1))[0][:8])
    assert np.array_equal(od, sd[:, :k1]), (tag, "the two references disagree")
    assert np.array_equal(fl != 0, _tie_flags(od)), (tag, "flags")
    assert set(np.unique(fl)) <= {0, 1}, (tag, np.unique(fl))
    assert np.array_equal(gi, si[:, :k1]), (tag, "ids by (distance, id)", np.nonzero((gi != si[:, :k1]).any(1))[0][:8])
    plain = fl == 0
    assert np.array_equal(gi[plain][:, :k1 - 1], oi[plain][:, :k1 - 1]), (tag, "ids")
    whole = plain & (sd[:, k1 - 1] != sd[:, k1])
    assert np.array_equal(gi[whole], oi[whole]), (tag, "ids")
    return fl


# ---------------------------------------------------------------------------------------------------- integer data
@pytest.mark.parametrize("dim", [1, 20, 100, 130, 384, 2048])  # dim_p / 16 = 1, 2, 7, 9, 24, 128
def test_integer_data_against_the_oracle(gpu_pkg, dim):
    rng = np.random.default_rng(11000 + dim)
    n = 20000
    base, q = _int_data(rng, n, 48, dim)
    seen = set()
    sref = _sorted_int_ref(base, q, 17)
    with gpu_pkg.BruteForceIndex(base) as idx:
        for k in KS:
            oi, od = oracle.search_bf(base, q, k + 1)
            for call, nb, B in SHAPES:
                _on_route_2(gpu_pkg, n, dim, nb, B, k)
                fl = _check_int(tc._bf_dev(idx, q, nb, B, k, call), oi[:nb * B], od[:nb * B], sref, (dim, k, call, nb, B))
                seen |= set(fl.tolist())
    assert seen == ({0, 1} if dim >= 20 else {1})  # (256 values of one coordinate in 20 000 rows: every query ties)


@pytest.mark.parametrize("dim", [100, 960])
@pytest.mark.parametrize("n", [1, 5, 17, 63, 64, 65, 4099])
def test_ragged_bases(gpu_pkg, dim, n):
    rng = np.random.default_rng(12000 + dim + n)
    base, q = _int_data(rng, n, 7, dim, dup=0.05 if n > 1000 else 0.0)  # (the planted copies need 160 rows and more)
    if n >= 2:
        base[n - 1] = base[0]
        q[0] = base[0]
    k = 5
    wi, wd = _sorted_int_ref(base, q, k + 1)
    assert (n > k) or ((wi[:, n:] == -1).all() and np.isposinf(wd[:, n:]).all())
    _on_route_2(gpu_pkg, n, dim, 1, 7, k)
    with gpu_pkg.BruteForceIndex(base) as idx:
        gi, gd, fl = tc._bf_dev(idx, q, 1, 7, k, "one")
    assert np.array_equal(gd, wd), (n, dim)
    want_fl = (np.isfinite(wd[:, 1:]) & (wd[:, 1:] == wd[:, :-1])).any(1)
    assert np.array_equal(fl != 0, want_fl)
    assert np.array_equal(gi, wi)  # ((distance, id) order: equal also where a flag is set)
    assert n < 2 or fl[0] == 1


def test_every_wave_works_several_units(gpu_pkg):
    """dim 20, B = 16, k = 15 on a base of three complete runs of units (every wave works three: the checkpoints and the
    bounded insertion are in use) and on one of two complete runs and an incomplete third.  Both directions."""
    k, B = 15, 16
    grid, unit = gpu_pkg.BruteForceIndex.one_plan(10 ** 7, 20, _cus(), 1, B, k)[1:3]
    run = grid * 8 * unit
    for n, tag in ((3 * run, "complete"), (2 * run + 70, "incomplete")):
        plan = _on_route_2(gpu_pkg, n, 20, 1, B, k)
        assert plan[1] == grid and plan[3] == 3, plan
        rng = np.random.default_rng(13000 + (n % 1000))
        base, q = _int_data(rng, n, B, 20)
        oi, od = oracle.search_bf(base, q, k + 1)
        sref = _sorted_int_ref(base, q, k + 2)
        with gpu_pkg.BruteForceIndex(base) as idx:
            for rep in range(2):
                fl = _check_int(tc._bf_dev(idx, q, 1, B, k, "one"), oi, od, sref, (tag, rep))
        assert set(fl.tolist()) == {0, 1}, tag


# ---------------------------------------------------------------------------------------------------- cancelling distances
def _check_cancel(idx, key, nb, B, k, call, tag, require):
    """tc._check_dev; for the shapes too small to hold a negative distance, a +0 and a tie, without that precondition"""
    if require:
        return tc._check_dev(idx, key, nb, B, k, call, tag)
    q = cancel_data.case(*key)[1]
    ri, rd = tc._sorted_ref(key)
    n = nb * B
    wi, wd = ri[:n, :k + 1], rd[:n, :k + 1]
    gi, gd, fl = tc._bf_dev(idx, q, nb, B, k, call)
    tc._assert_same((gi, gd), (wi, wd), (tag, call, nb, B, k))
    assert np.array_equal(fl, tc._flags(wd)), (tag, call, nb, B, k)
    return gi, gd, fl


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("dim", [20, 100, 384])
def test_real_valued_data_where_distances_cancel(gpu_pkg, dim, offset):
    key = (20000, 96, dim, offset)
    with gpu_pkg.BruteForceIndex(cancel_data.case(*key)[0]) as idx:
        for k in KS:
            for call, nb, B in SHAPES:
                _on_route_2(gpu_pkg, key[0], dim, nb, B, k)
                # (the first 16 queries of the 384-d set at offset 4 hold no +0 at k = 1: the precondition goes with the
                # 48-query calls, on every set)
                _check_cancel(idx, key, nb, B, k, call, f"nd one {dim}", require=nb * B == 48)


# ---------------------------------------------------------------------------------------------------- inner product
@pytest.mark.parametrize("dim", [100, 768])
@pytest.mark.parametrize("name", ["signed", "zeros"])
def test_inner_product(gpu_pkg, name, dim):
    """the float64 product on integer data (test_gpu_ip.py's sets); `zeros`: all-zero queries and queries orthogonal to
    planted rows -- an exactly zero product comes back as -0.0"""
    n = 20000
    base, q = tip._data(name, n, 48, dim)
    ref = tip._ref(name, n, 48, dim)
    with gpu_pkg.BruteForceIndex(base, metric=gpu_pkg.METRIC_IP) as idx:
        for k in (5, 15):
            for call, nb, B in SHAPES:
                _on_route_2(gpu_pkg, n, dim, nb, B, k)
                got = tip._dev_call(idx, q, nb, B, k, "dev" if call == "one" else "multi")
                wi, wd, wf = tip._expect(ref, nb * B, k)
                tip._assert_lists(got, (wi, wd, wf), f"{name} {dim} {call} nb={nb} B={B} k={k}")
                zero = wd == 0
                assert (bits(got[1])[zero] == np.int32(-2 ** 31)).all(), "a zero product is -0.0"
                if name == "zeros" and nb * B >= 16:
                    assert zero[list(tip.ORTH_QUERIES)].any(1).all() and zero[0].all()


# ---------------------------------------------------------------------------------------------------- properties of the route
def _all_calls(idx, q, ks=KS):
    return {(k, call, nb, B): tc._bf_dev(idx, q, nb, B, k, call) for k in ks for call, nb, B in SHAPES}


def _same_bits(a, b):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("dim", [100, 768])
def test_result_does_not_depend_on_the_route(gpu_pkg, dim):
    """two indexes on the same rows in one process, the second created under VSEARCH_ND_ONE=0 (the per-batch scan)"""
    if dim == 100:
        base, q, _ = cancel_data.case(20000, 96, 100, 4)
    else:
        base, q = _int_data(np.random.default_rng(14000), 20000, 48, dim)
    for k in KS:
        for call, nb, B in SHAPES:
            _on_route_2(gpu_pkg, len(base), dim, nb, B, k)
    with gpu_pkg.BruteForceIndex(base) as one:
        old = os.environ.get("VSEARCH_ND_ONE")
        os.environ["VSEARCH_ND_ONE"] = "0"
        try:
            per_batch = gpu_pkg.BruteForceIndex(base)
        finally:
            if old is None:
                del os.environ["VSEARCH_ND_ONE"]
            else:
                os.environ["VSEARCH_ND_ONE"] = old
        with per_batch:
            a, b = _all_calls(one, q), _all_calls(per_batch, q)
    for key in a:
        assert _same_bits(a[key], b[key]), (dim, key)
    assert any(x[2].any() for x in a.values()) and any((x[2] == 0).any() for x in a.values())


def test_same_call_repeated(gpu_pkg):
    """four times in a row: both directions of the walk, and the arrival counter is back at its start value each time"""
    base, q, _ = cancel_data.case(20000, 96, 384, 4)
    _on_route_2(gpu_pkg, len(base), 384, 3, 16, 5)
    with gpu_pkg.BruteForceIndex(base) as idx:
        runs = [tc._bf_dev(idx, q, 3, 16, 5, "multi") for _ in range(4)]
        runs += [tc._bf_dev(idx, q, 1, 16, 5, "one") for _ in range(4)]
    for r in runs[1:4]:
        assert _same_bits(runs[0], r)
    for r in runs[4:]:
        assert _same_bits(tuple(x[:16] for x in runs[0]), r)
    ri, rd = tc._sorted_ref((20000, 96, 384, 4))
    tc._assert_same(runs[0][:2], (ri[:48, :6], rd[:48, :6]), "repeated")


def test_id_offset(gpu_pkg):
    rng = np.random.default_rng(15000)
    base, q = _int_data(rng, 5000, 16, 100)
    base[4998] = base[0]  # fewer real rows than k + 1 never happens here: every id is a row's
    _on_route_2(gpu_pkg, 5000, 100, 1, 16, 5)
    wi, wd = _sorted_int_ref(base, q, 6, id_offset=1000)
    with gpu_pkg.BruteForceIndex(base, id_offset=1000) as idx:
        gi, gd, fl = tc._bf_dev(idx, q, 1, 16, 5, "one")
    assert np.array_equal(gd, wd) and np.array_equal(gi, wi) and gi.min() >= 1000


def test_uint8_index(gpu_pkg):
    """precision 0: byte-valued queries stay on the byte scan (a batch with a value that is no byte is skipped by it:
    flags == 2), results unchanged.  Precision 1: the fp32 rows, on the single-call route: the fp32 index's answer."""
    rng = np.random.default_rng(16000)
    n, dim, B, k = 20000, 100, 16, 5
    base, q = _int_data(rng, n, B, dim)
    _on_route_2(gpu_pkg, n, dim, 1, B, k)
    oi, od = oracle.search_bf(base, q, k + 1)
    bad = q.copy()
    bad[3, 7] = 0.5
    with gpu_pkg.BruteForceIndex(base) as f32:
        want = tc._bf_dev(f32, q, 1, B, k, "one")
        want_bad = tc._bf_dev(f32, bad, 1, B, k, "one")
    sref = _sorted_int_ref(base, q, k + 2)
    _check_int(want, oi, od, sref, "fp32 index")
    with gpu_pkg.BruteForceIndex.from_u8(base.astype(np.uint8)) as idx:
        _check_int(tc._bf_dev(idx, q, 1, B, k, "one"), oi, od, sref, "byte scan")
        assert (tc._bf_dev(idx, bad, 1, B, k, "one")[2] == 2).all()  # the byte scan's verdict: this call is not rerouted
        idx.set_precision(1)
        assert _same_bits(tc._bf_dev(idx, q, 1, B, k, "one"), want)
        assert _same_bits(tc._bf_dev(idx, bad, 1, B, k, "one"), want_bad)
        assert _same_bits(tc._bf_dev(idx, q, 1, 7, k, "one"), tuple(x[:7] for x in want))


def test_general_index_at_128_equals_the_specialised_kernel(gpu_pkg, tmp_path):
    """VSEARCH_ND_FORCE=1 in a child process: scan_one_nd_kernel at dim 128 against scan_one_kernel here"""
    out = str(tmp_path / "forced.npz")
    r = subprocess.run([sys.executable, os.path.abspath(nd_one_child.__file__), ROOT, out], env=dict(os.environ, VSEARCH_ND_FORCE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ND_ONE_CHILD_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1500:])
    forced = np.load(out)
    assert os.environ.get("VSEARCH_ND_FORCE", "0") == "0"
    here = nd_one_child.run(gpu_pkg, 1)
    ri, rd = tc._sorted_ref(nd_one_child.KEY)
    for k in nd_one_child.KS:
        assert np.array_equal(forced[f"i{k}"], here[f"i{k}"]), k
        assert np.array_equal(bits(forced[f"d{k}"]), bits(here[f"d{k}"])), k
        assert np.array_equal(forced[f"f{k}"], here[f"f{k}"]), k
        tc._assert_same((forced[f"i{k}"], forced[f"d{k}"]), (ri[:, :k + 1], rd[:, :k + 1]), ("forced", k))
