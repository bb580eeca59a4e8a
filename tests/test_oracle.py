"""The CPU oracle against (a) the reference outputs recorded by the survey run of the unmodified
cpu_baseline.cpp (tests/golden/PROVENANCE.md) and (b) an independent int64 recomputation."""
import os

import numpy as np
import pytest

import oracle


def _load_ref(golden_dir, tag):
    b = oracle.read_fvecs(os.path.join(golden_dir, f"ref_ties_{tag}_base.fvecs"))
    q = oracle.read_fvecs(os.path.join(golden_dir, f"ref_ties_{tag}_query.fvecs"))
    ids, d = oracle.parse_results_txt(os.path.join(golden_dir, f"ref_ties_{tag}_results.txt"))
    return b, q, np.array(ids, dtype=np.int32), np.array(d, dtype=np.float32)


@pytest.mark.parametrize("tag", ["fwd", "rev"])
def test_tie_probe_matches_reference(golden_dir, tag):
    # select_topk's history-dependent tie order
    b, q, rid, rd = _load_ref(golden_dir, tag)
    ids, d = oracle.search_bf(b, q, 5)
    assert np.array_equal(ids, rid)
    assert np.array_equal(d, rd)
    if tag == "fwd":
        assert ids[0].tolist() == [5, 7, 2, 3, 4]
    else:
        assert ids[0].tolist() == [1, 3, 0, 2, 4]


def test_synth10k_matches_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "ref_synth10k_inputs.npz"))
    base, query = z["base"].astype(np.float32), z["query"].astype(np.float32)
    rid, rd = oracle.parse_results_txt(os.path.join(golden_dir, "ref_synth10k_results.txt"))
    ids, d = oracle.search_bf(base, query, 5)
    assert np.array_equal(ids, np.array(rid))
    assert np.array_equal(d, np.array(rd, dtype=np.float32))  # all < 1e6, so "%g" printed them exactly
    # independent pin: exact integer arithmetic
    ex = oracle.exact_int_dists(query, base)
    assert np.array_equal(np.sort(ex, axis=1)[:, :5].astype(np.float32), d)
    assert np.array_equal(ex[np.arange(len(ids))[:, None], ids].astype(np.float32), d)


def test_norms_and_distances_exact_on_integer_data():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 219, size=(777, 128)).astype(np.float32)
    q = rng.integers(0, 219, size=(9, 128)).astype(np.float32)
    assert np.array_equal(oracle.compute_norms(base), (base.astype(np.int64) ** 2).sum(1).astype(np.float32))
    ex = oracle.exact_int_dists(q, base)
    for i in range(len(q)):
        assert np.array_equal(oracle.l2_row(q[i], base), ex[i].astype(np.float32))


def test_select_topk_slot_semantics():
    # crafted: first slot holding the max is replaced; equal distance never replaces (strict <)
    d = np.array([100, 100, 100, 100, 100, 9, 100, 9, 100], dtype=np.float32)
    idx, dd = oracle.select_topk(d, 5)
    assert idx.tolist() == [5, 7, 2, 3, 4]
    assert dd.tolist() == [9, 9, 100, 100, 100]
    # descending ids among ties are possible: slot 1 is replaced first, slot 0 later
    d = np.array([50, 60, 1, 2, 3, 7, 7], dtype=np.float32)
    idx, dd = oracle.select_topk(d, 5)
    # slots: [50,60,1,2,3] -> max slot1 <- (7,id5) -> [50,7,1,2,3] -> max slot0 <- (7,id6)
    assert idx.tolist() == [2, 3, 4, 6, 5]
    # k > N clamps
    idx, dd = oracle.select_topk(np.array([3, 1], dtype=np.float32), 4)
    assert idx.tolist() == [1, 0, -1, -1] and np.isinf(dd[2:]).all()


def test_sparse_slots_equal_dense():
    rng = np.random.default_rng(1)
    for trial in range(50):
        n = int(rng.integers(6, 400))
        d = rng.integers(0, 12, size=n).astype(np.float32)  # many ties
        k = int(rng.integers(1, 6))
        di, dd = oracle.select_topk(d, k)
        # candidate superset: the first k rows plus every row below the running k-th value of its prefix
        keep = list(range(min(k, n)))
        for j in range(k, n):
            if d[j] < np.sort(d[:j])[k - 1]:
                keep.append(j)
        keep = np.array(keep, dtype=np.int32)
        si, sd = oracle.select_topk_sparse(keep, d[keep], k)
        assert np.array_equal(di, si) and np.array_equal(dd, sd)


def test_read_fvecs_errors(tmp_path):
    p = tmp_path / "t.fvecs"
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    rec = np.concatenate([np.full((3, 1), 4, dtype=np.int32).view(np.float32), x], axis=1)
    rec.tofile(p)
    assert np.array_equal(oracle.read_fvecs(str(p)), x)
    with open(p, "ab") as f:
        f.write(b"\x04\x00")  # truncated trailing record (cpu_baseline.cpp:53-56)
    with pytest.raises(IOError):
        oracle.read_fvecs(str(p))
    with pytest.raises(IOError):
        oracle.read_fvecs(str(tmp_path / "missing.fvecs"))


def test_ivf_oracle_full_probe_equals_exact():
    rng = np.random.default_rng(2)
    base = rng.integers(0, 219, size=(3000, 128)).astype(np.float32)
    q = rng.integers(0, 219, size=(20, 128)).astype(np.float32)
    nlist = 24
    cents = base[rng.choice(len(base), nlist, replace=False)] + 0.25
    d = (base ** 2).sum(1)[:, None] - 2 * base @ cents.T + (cents ** 2).sum(1)[None]
    assign = d.argmin(1)
    order = np.argsort(assign, kind="stable").astype(np.int32)
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    ids, dd, total = oracle.ivf_search(base[order], off, order, cents, q, 5, nlist)
    ex = oracle.exact_int_dists(q, base)
    assert total == len(q) * len(base)
    assert np.array_equal(dd, np.sort(ex, 1)[:, :5].astype(np.float32))
    assert np.array_equal(ex[np.arange(len(q))[:, None], ids].astype(np.float32), dd)
    # fewer probes: recall definition of main_ivf.cpp:52-59
    ids8, _, total8 = oracle.ivf_search(base[order], off, order, cents, q, 5, 8)
    assert total8 < total
    r = oracle.recall(ids8, ids, 5)
    assert 0.0 <= r <= 1.0
    assert oracle.recall(ids, ids, 5) == 1.0


def test_q8_quantiser_known_answers_and_numpy_recomputation():
    """quantize_buffer_neon (QnnRunner.cpp:13-55) by hand: x / 0.6627451 + 0.5, towards zero, saturated to [0, 255];
    then the whole uint8 score path against a numpy recomputation with separately rounded fp32 products and sums."""
    x = np.array([0.0, 0.33, 0.34, 1.0, -3.0, 200.0, 1e9, np.nan, 0.6627451 * 2.5, 168.8, 169.1], dtype=np.float32)
    assert oracle.q8_quantize(x, oracle.Q8_INPUT_SCALE).tolist() == [0, 0, 1, 2, 0, 255, 255, 0, 3, 255, 255]
    assert oracle.q8_quantize_weights(np.array([-2.0, 0.0, 2.0, 300.0], dtype=np.float32), 1.0, -3).tolist() == [3, 3, 5, 255]
    rng = np.random.default_rng(5)
    base = (rng.random((700, 128)) * 90).astype(np.float32)
    q = (rng.random((9, 128)) * 170).astype(np.float32)
    i_s, w_s, off, o_s = 0.6627451, 0.4, -7, 3000.0
    got = oracle.q8_scores(base, q, i_s, w_s, off, o_s)
    inv_i, inv_w = np.float32(1) / np.float32(i_s), np.float32(1) / np.float32(w_s)
    q8 = np.clip(np.trunc(q * inv_i + np.float32(0.5)), 0, 255).astype(np.int64)
    w8 = np.clip(np.clip(np.trunc(base * inv_w + np.float32(0.5)), 0, 255).astype(np.int64) - off, 0, 255)
    ip = q8 @ (w8 + off).T
    mult = (np.float32(i_s) * np.float32(w_s)) / np.float32(o_s)
    want = np.clip(np.trunc(ip.astype(np.float32) * mult + np.float32(0.5)), 0, 255).astype(np.uint8)
    assert np.array_equal(got, want) and len(np.unique(want)) > 10
    ids, top = oracle.q8_topk(got, 6)
    for b in range(len(q)):
        order = np.lexsort((np.arange(got.shape[1]), -got[b].astype(np.int64)))[:6]
        assert ids[b].tolist() == order.tolist() and top[b].tolist() == got[b][order].tolist()
    ids, top = oracle.q8_topk(got[:, :4], 6)  # fewer rows than k (IVFIndex.cpp:457 clamps likewise): (-1, 0) tail
    assert np.all(ids[:, 4:] == -1) and np.all(top[:, 4:] == 0)


# ---------------------------------------------------------------------------------------------------------------------
# dot orders: "chain" (the product's fp32 MFMA kernels) and "fold8" (the query-major IVF list scan) beside "lanes8"
# ---------------------------------------------------------------------------------------------------------------------
def _chain_index_order(dim):
    return [16 * c + 4 * g + i for c in range((dim + 15) // 16) for i in range(4) for g in range(4) if 16 * c + 4 * g + i < dim]


def _fma_chain(a, b, order):
    """acc = fmaf(a[x], b[x], acc) over `order`, one rounding per step: the product of two fp32 numbers is exact in
    float64, and the float64 sum of that product and an fp32 accumulator rounded to fp32 is the fused result unless the
    float64 sum itself had to round -- which the callers' inputs (few significant bits) rule out."""
    acc = np.float32(0)
    for x in order:
        s = np.float64(a[x]) * np.float64(b[x]) + np.float64(acc)
        acc = np.float32(s)
    return acc


@pytest.mark.parametrize("dim", [1, 3, 20, 100, 128, 130, 300])
def test_dot_orders_are_exact_on_integer_data(dim):
    rng = np.random.default_rng(dim)
    base = rng.integers(0, 219, size=(200, dim)).astype(np.float32)
    q = rng.integers(0, 219, size=(5, dim)).astype(np.float32)
    ex = oracle.exact_int_dists(q, base).astype(np.float32)
    for order in ("lanes8", "chain", "fold8"):
        assert np.array_equal(oracle.l2_matrix(q, base, order), ex), order
        ids, d = oracle.search_bf(base, q, 5, dot_order=order)
        ids0, d0 = oracle.search_bf(base, q, 5)
        assert np.array_equal(ids, ids0) and np.array_equal(d, d0), order


@pytest.mark.parametrize("dim", [1, 7, 20, 100, 128, 960, 2048])
def test_dot_orders_within_gamma_of_float64(dim):
    """Any fp32 summation of dim products, fused or not, stays within gamma_dim * sum |a b| of the true value
    (gamma_n = n u / (1 - n u), u = 2^-24: Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
    rng = np.random.default_rng(100 + dim)
    a = rng.standard_normal((50, dim)).astype(np.float32)
    b = rng.standard_normal((50, dim)).astype(np.float32)
    u = 2.0 ** -24
    gamma = dim * u / (1 - dim * u)
    for order in ("lanes8", "chain", "fold8"):
        for i in range(len(a)):
            got = float(oracle.dot(a[i], b[i], order))
            true = float(a[i].astype(np.float64) @ b[i].astype(np.float64))
            bound = gamma * float(np.abs(a[i].astype(np.float64) * b[i].astype(np.float64)).sum())
            assert abs(got - true) <= bound, (order, dim, i, got, true, bound)


def test_chain_order_by_hand_on_20_elements():
    """b = 1; a holds one 2^24 (element 0), one -2^24 and ones.  A 1 added to +-2^24 is lost (ties to even), a 1 added to
    anything smaller survives: the result counts the ones that an order visits outside the stretch between the two big
    elements.  Visiting orders of the 20 elements: chain = 0 4 8 12 | 1 5 9 13 | 2 6 10 14 | 3 7 11 15 | 16 17 18 19,
    ascending = 0 1 2 ... 19 (the ones at 1 .. 8 are lost, 10 survive), lanes8 = lane j sums j and j + 8 (r0 = 2^24: one
    lost, r1 = 1 - 2^24 exact, the others 2), the lanes are added pairwise (1 + 4 + 8 = 13), then the tail 16 .. 19: 17."""
    a = np.ones(20, dtype=np.float32)
    b = np.ones(20, dtype=np.float32)
    a[0] = 2.0 ** 24
    a[9] = -2.0 ** 24     # chain position 6: the ones at 4, 8, 12, 1, 5 are lost, the 13 after it survive
    chain = _fma_chain(a, b, _chain_index_order(20))
    asc = _fma_chain(a, b, range(20))
    # lanes8 by hand: lanes r[j] = a[j] + a[j + 8] (exact, fmaf), ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), tail
    r = [np.float32(np.float64(a[j]) + np.float64(a[j + 8])) for j in range(8)]
    f = lambda x, y: np.float32(np.float64(x) + np.float64(y))
    l8 = f(f(f(r[0], r[1]), f(r[2], r[3])), f(f(r[4], r[5]), f(r[6], r[7])))
    for x in range(16, 20):
        l8 = f(l8, a[x])
    assert (float(chain), float(asc), float(l8)) == (13.0, 10.0, 17.0)
    assert oracle.dot(a, b, "chain") == chain
    assert oracle.dot(a, b, "lanes8") == l8
    # the same numbers through math.fma where the interpreter has it (3.13+): double rounding cannot occur here
    import math
    if hasattr(math, "fma"):
        acc = 0.0
        for x in _chain_index_order(20):
            acc = float(np.float32(math.fma(float(a[x]), float(b[x]), acc)))
        assert acc == 13.0
    # fold8: lane s walks 4s .. 4s + 3 (only m = 0 exists below 32): p0 = 2^24 (three ones lost), p1 = 4, p2 = 1 - 2^24 + 1 + 1
    # = -2^24 + 3 (exact: the spacing below 2^24 is 1), p3 = p4 = 4, p5 = p6 = p7 = 0: ((2^24 + 4) + (-2^24 + 7)) + (4 + 0) = 15
    assert float(oracle.dot(a, b, "fold8")) == 15.0


def test_chain_order_on_random_fp32_equals_the_python_chain():
    """random 11-bit mantissas: every product has <= 22 bits and the float64 accumulation step of _fma_chain is exact"""
    rng = np.random.default_rng(7)
    for dim in (1, 3, 20, 100, 130):
        a = (rng.integers(-1023, 1024, dim) * 2.0 ** rng.integers(-6, 6, dim)).astype(np.float32)
        b = (rng.integers(-1023, 1024, dim) * 2.0 ** rng.integers(-6, 6, dim)).astype(np.float32)
        assert oracle.dot(a, b, "chain") == _fma_chain(a, b, _chain_index_order(dim)), dim
    differs = 0
    for _ in range(50):
        a = rng.standard_normal(100).astype(np.float32)
        b = rng.standard_normal(100).astype(np.float32)
        differs += oracle.dot(a, b, "chain") != oracle.dot(a, b, "lanes8")
    assert differs >= 10   # the two orders are different functions on ordinary data


def test_norm_tail_is_a_fused_multiply_add():
    """dims that are no multiple of 8: the tail of the squared norm is fmaf(v, v, sum), as in the kernels' prep code,
    whatever -ffp-contract says.  Lanes: 64^2 + 64^2 = 8192 (spacing 2^-10 there).  Tail v = 1 + 2^-12, v^2 = 1 + 2^-11 +
    2^-24: fused, 8193 + 2^-11 + 2^-24 lies above the half-way point and rounds up to 8193 + 2^-10; with the product
    rounded first (to 1 + 2^-11, ties to even) the sum is the exact half-way point and rounds to the even 8193."""
    v = np.zeros((1, 9), dtype=np.float32)
    v[0, 0] = v[0, 1] = 64.0
    v[0, 8] = np.float32(1 + 2.0 ** -12)
    assert oracle.compute_norms(v)[0] == np.float32(8193 + 2.0 ** -10)
    assert np.float32(np.float32(v[0, 8] * v[0, 8]) + np.float32(8192)) == np.float32(8193)  # the unfused tail differs


def test_ivf_oracle_orders_agree_on_integer_centroids_and_name_the_scan_order():
    rng = np.random.default_rng(3)
    base = rng.integers(0, 219, size=(3000, 128)).astype(np.float32)
    q = rng.integers(0, 219, size=(20, 128)).astype(np.float32)
    nlist = 24
    cents = base[rng.choice(len(base), nlist, replace=False)].copy()
    d = (base ** 2).sum(1)[:, None] - 2 * base @ cents.T + (cents ** 2).sum(1)[None]
    assign = d.argmin(1)
    order = np.argsort(assign, kind="stable").astype(np.int32)
    off = np.zeros(nlist + 1, dtype=np.int32)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    want = oracle.ivf_search(base[order], off, order, cents, q, 5, 4, return_probes=True)
    for kw in ({"dot_order": "chain"}, {"dot_order": "chain", "scan_order": "fold8"}, {"dot_order": "lanes8"}):
        got = oracle.ivf_search(base[order], off, order, cents, q, 5, 4, return_probes=True, **kw)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(got, want)), kw
    got = oracle.ivf_search(base[order], off, order, cents, q, 5, 4, dot_order="chain", return_coarse=True)
    assert got[4].shape == (20, 4) and (np.diff(got[4], axis=1) >= 0).all()
    ex = oracle.exact_int_dists(q, cents).astype(np.float32)
    assert np.array_equal(np.take_along_axis(ex, got[3].astype(np.int64), 1), got[4])


# ---------------------------------------------------------------------------------------------------------------------
# tests/cancel_data.py: self-queries on real-valued rows.  Asserted on the reference alone, for every data set that
# test_gpu_cancel.py searches, that the expected results hold what that data is for.  These are conditions on the data,
# not measurements of the product: a seed that misses one is replaced (cancel_data.SEED), no count is lowered.
# ---------------------------------------------------------------------------------------------------------------------
import cancel_data  # noqa: E402


@pytest.mark.parametrize("n,nq,dim,offset", cancel_data.BF_SETS)
def test_cancel_data_produces_negative_zero_and_tied_distances(n, nq, dim, offset):
    base, q, src = cancel_data.case(n, nq, dim, offset)
    m, mid = cancel_data.layout(n)
    assert np.array_equal(q, base[src]) and np.array_equal(base[n - m:], base[:m]) and np.array_equal(base[mid:mid + 50], base[:50])
    assert mid % 64 != 0 and (n - m) % 64 != 0  # a copy never sits at its original's place inside a 64-row block
    bounds = [n // 3 // 16 * 16, 2 * n // 3 // 16 * 16]           # three contiguous shards: copies on both sides of each border
    assert m < bounds[0] < mid and mid + 50 < bounds[1] < n - m
    ids, d = cancel_data.sorted_scores(q[:64], base, 17)
    # the self-query, its copies and the two planted neighbours are each query's five best and the rest is far away
    i = np.arange(len(ids))
    want = [{int(s), int(n - m + s), int(m + 3 * j + 1), int(n - m - 2 - 5 * j)} | ({int(mid + s)} if s < 50 else set()) for j, s in zip(i, src[:64])]
    assert all(set(ids[j, :len(want[j])].tolist()) == want[j] for j in i)
    assert (d[i, [len(w) for w in want]] > 1).all() and (d[i, [len(w) - 1 for w in want]] < 1e-4 * dim * (1 + offset) ** 2).all()
    neg, zero, tie, _ = cancel_data.require(d, 5, f"n {n} dim {dim} offset {offset}", negative=8, zero=4, tie=32)
    assert max(cancel_data.counts(d, k)[3] for k in (1, 5, 15)) >= 1  # some tested k has a negative k-th best: a bound below 0


@pytest.mark.parametrize("n,nq,dim,offset,nlist", cancel_data.IVF_SETS)
def test_cancel_ivf_layout_produces_negative_and_zero_coarse_scores(n, nq, dim, offset, nlist):
    vr, off, r2o, cents, q = cancel_data.ivf_case(n, nq, dim, offset, nlist)
    base = cancel_data.case(n, nq, dim, offset)[0]
    assert np.array_equal(vr, base[r2o]) and off[0] == 0 and off[-1] == n and len(np.unique(cents, axis=0)) == nlist
    assert len(q) == nq + nlist // 2 and np.array_equal(q[nq:], cents[::2])
    lists = np.repeat(np.arange(nlist), np.diff(off))
    assert (np.diff(lists) >= 0).all() and all((np.diff(r2o[off[c]:off[c + 1]]) > 0).all() for c in range(nlist))  # stable
    score = oracle.l2_matrix(cents, base, "chain")
    assert np.array_equal(lists, score.argmin(0)[r2o])
    q = q[:256]
    wide = nlist <= 64
    cases = {64: ((1, 1), (10, 8), (16, 8), (2, 1), (3, 8), (17, 8), (100, 8)), 24: ((1, 1), (10, 4), (16, 8), (40, 8), (128, 24)),
             5000: ((1, 24), (5, 24))}[nlist]
    neg_kth = 0
    for k, nprobe in cases:
        scan = "fold8" if nlist > 4096 else None
        _, od, _, _, coarse = oracle.ivf_search(vr, off, r2o, cents, q, k + 1, nprobe, dot_order="chain", scan_order=scan, return_coarse=True)
        c = cancel_data.require(od[:64], k, f"ivf n {n} dim {dim} offset {offset} nlist {nlist} k {k} nprobe {nprobe}",
                                negative=8, zero=4, tie=32 if (k > 1 or not wide) and nprobe > 1 else 1)
        neg_kth += c[3]
        assert int((coarse < 0).sum()) >= 4 and int(((coarse == 0) & ~np.signbit(coarse)).sum()) >= 4, (k, nprobe)
    assert neg_kth >= 1


def test_results_writer_on_cancelled_distances(pkg, tmp_path):
    """a tiny negative, +0, a denormal and (-1, +inf) padding: the default form is "%g"'s, the fixed four-decimal form
    prints the tiny negative as -0.0000, as std::fixed does in the reference's writer"""
    d = np.array([[-7.6293945e-06, 0.0, 2.0 ** -140, np.inf], [0.0, 0.0, 0.00015, np.inf]], dtype=np.float32)
    ids = np.array([[3, 19999, 7, -1], [0, 1, 2, -1]], dtype=np.int32)
    assert d[0, 0] < 0 and 0 < d[0, 2] < np.finfo(np.float32).tiny
    p, po = str(tmp_path / "p.txt"), str(tmp_path / "o.txt")
    pkg.write_results(p, ids, d)
    oracle.write_results(po, ids, d)
    assert open(p).read() == open(po).read() == "Query 0: (3, -7.62939e-06) (19999, 0) (7, 7.17465e-43)\nQuery 1: (0, 0) (1, 0) (2, 0.00015)\n"
    pkg.write_results(p, ids, d, style=1)
    assert open(p).read() == "Query 0: (3, -0.0000) (19999, 0.0000) (7, 0.0000)\nQuery 1: (0, 0.0000) (1, 0.0000) (2, 0.0002)\n"
    assert open(p).read().split()[3] == "%.4f)" % d[0, 0]
    pkg.write_results(p, ids, d)  # the fixed form of one call does not leak into the next
    assert open(p).read() == open(po).read()
