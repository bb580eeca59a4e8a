"""Wide-k brute force (16 <= k <= 128) on the byte rows of a general index made from uint8 rows (scan_nd_i8_wide_kernel,
DESIGN 4.5c) against the CPU references.

Reference: under squared L2 oracle.search_bf on the rows as float (exact on nd_u8_data: integers, every squared norm under
2^23), under inner product nd_u8_ip_data.topk_ref over the int64 products.  Secondary, every result of the byte route also
equals the same index under set_precision(1), the fp32 launches.  Every case asserts through wide_stats() that the
batches it means ran on the byte rows before it compares anything.  P(k) is read from wide_plan, never hard-coded."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import nd_u8_ip_data as D  # noqa: E402
import nd_wide_u8_child as child  # noqa: E402
import oracle  # noqa: E402
from nd_u8_data import sqnorm_max, u8_data  # noqa: E402

pytestmark = pytest.mark.gpu

NQ, B = 40, 20
CAP = 8192
dev_topk = child.dev_topk


def _f32(a):
    return a.astype(np.float32)


def P(pkg, k, dim=96, n=10 ** 5):
    on_bytes, rows, cap = pkg.BruteForceIndex.wide_plan(n, dim, k)
    assert on_bytes == 1 and cap == CAP
    return rows


def _l2_data(seed, n, nq, dim):
    """u8_data, and queries 8.. that ARE rows of the end of the base: their best rows lie behind the prefix"""
    base, q = u8_data(np.random.default_rng(seed), n, nq, dim)
    for j in range(min(4, nq - 8, n)):
        q[8 + j] = base[n - 1 - 3 * j % n]
    return base, q


def _ids_by_id_order(dist, oi, od, rows):
    """The ids a device call owes for the queries `rows`, none of which has two equal distances among its od: in every
    column the smallest id at that distance of dist [nq, n], since the scans order equal distances by id (the last of the
    k + 1 may be tied with a row beyond them; the reference's slot order keeps either)."""
    want = np.array(oi, copy=True)
    for i in rows:
        for j in range(od.shape[1]):
            if np.isfinite(od[i, j]):
                want[i, j] = np.flatnonzero(dist[i] == od[i, j])[0]
        assert np.array_equal(want[i, :-1], oi[i, :-1])
    return want


def _cand_behind(dist_row, prefix, k1):
    """rows behind the prefix under tau = next_up(k1-th best of the prefix): what the filter pass keeps for this query"""
    kth = np.sort(dist_row[:prefix])[k1 - 1]
    return int((dist_row[prefix:] < np.nextafter(np.float32(kth), np.float32(np.inf))).sum())


def _same_bits(got, want):
    """float arrays equal bit for bit (-0.0 is not 0.0); the first differences are reported"""
    a, b = np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(want).view(np.int32)
    bad = np.argwhere(a != b)
    assert bad.size == 0, [(tuple(ix), float(got[tuple(ix)]), float(want[tuple(ix)]), hex(a[tuple(ix)] & 0xffffffff)) for ix in bad[:8]]
    return True


class Moved:
    """with Moved(idx, (a, b, c)): the three counters of wide_stats move by exactly that"""

    def __init__(self, idx, by):
        self.idx, self.by = idx, by

    def __enter__(self):
        self.before = self.idx.wide_stats()

    def __exit__(self, *exc):
        if exc[0] is None:
            after = self.idx.wide_stats()
            assert tuple(a - b for a, b in zip(after, self.before)) == tuple(self.by), (self.before, after, self.by)


def _check_l2(pkg, base, q, k, nb=None, Bq=B, id_offset=0, host=True, want_ties=True):
    """device call (ids, distance bits, tie flags) and host call (ids, distances, the tie replay) on the byte route
    against oracle.search_bf, then against precision 1 of the same index"""
    n, nq = len(base), len(q)
    nb = nb or len(q) // Bq
    bf, qf = _f32(base), _f32(q)
    k1 = k + 1
    m = min(k1, n)
    oi1, od1 = oracle.search_bf(bf, qf[:nb * Bq], m)
    dist = oracle.l2_matrix(qf[:nb * Bq], bf)
    prefix = pkg.BruteForceIndex.wide_plan(n, base.shape[1], k)[1]
    if prefix < n:
        cand = [_cand_behind(row, prefix, k1) for row in dist]
        assert max(cand) <= CAP and sum(cand) > 0, "the filter pass is meant to find rows, and no list to overflow"
    ties = (od1[:, 1:] == od1[:, :-1]).any(1)
    wi = _ids_by_id_order(dist, oi1, od1, np.flatnonzero(~ties))
    with pkg.BruteForceIndex.from_u8(base, id_offset=id_offset) as idx:
        idx.set_batch(Bq)
        with Moved(idx, (nb, 0, nb)):
            ids, d, fl = dev_topk(idx, qf, nb, Bq, k)
        assert _same_bits(d[:, :m], od1)
        assert np.isposinf(d[:, m:]).all() and (ids[:, m:] == -1).all()
        assert not (fl == 2).any() and np.array_equal(fl != 0, ties)
        assert np.array_equal(ids[~ties, :m], wi[~ties] + id_offset)
        if host:
            hb = -(-nq // Bq)
            mh = min(k, n)
            oi, od = oracle.search_bf(bf, qf, mh)
            tm = pkg.Timing()
            with Moved(idx, (hb, 0, hb)):
                hi, hd = idx.search_topk(qf, k, tm)
            assert np.array_equal(hd[:, :mh], od) and np.array_equal(hi[:, :mh], oi + id_offset)
            assert np.isposinf(hd[:, mh:]).all() and (hi[:, mh:] == -1).all()
            if want_ties:
                assert tm.tie_queries > 0, "the tie replay did not run"
        idx.set_precision(1)
        with Moved(idx, (0, 0, nb)):
            ids1, d1, fl1 = dev_topk(idx, qf, nb, Bq, k)
        assert np.array_equal(ids, ids1) and _same_bits(d, d1) and np.array_equal(fl, fl1)
        if host:
            h1 = idx.search_topk(qf, k)
            assert np.array_equal(hi, h1[0]) and np.array_equal(hd, h1[1])


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 96, 129, 192, 200, 960, 2048])
def test_every_step_shape_l2(gpu_pkg, dim):
    """Odd and even counts of 64-byte steps, padded and unpadded tails, k = 16; behind the prefix three full 64-row blocks
    and a ragged one of 17.  Two batches of 20 on the device, the host call with its tie replay."""
    k = 16
    n = P(gpu_pkg, k, dim) + 209
    base, q = _l2_data(50000 + dim, n, NQ, dim)
    _check_l2(gpu_pkg, base, q, k)


@pytest.mark.parametrize("dim", [1, 64, 96, 128, 200, 2048])
def test_inner_product(gpu_pkg, dim):
    """The planted zero query, orthogonal rows and tied rows: zero scores and all-tied lists through both passes.

    The passes compute -0.0 for a zero product, as the fp32 passes do; the selection behind them (topk_wide_kernel) ranks
    -0 with +0 and has always returned +0.0 for either.  So the scores are compared with the reference as numbers, and
    bit for bit -- the sign of a zero included -- with precision 1 of the same index, the fp32 launches."""
    k = 16
    k1 = k + 1
    prefix = P(gpu_pkg, k, dim)
    n = prefix + 209
    base, q = D.ip_data(np.random.default_rng(51000 + dim), n, NQ, dim)
    ip = D.ip_int64(q, base)
    ri, rd = D.topk_ref(ip, k1)
    dist = -(ip.astype(np.float32))
    assert _cand_behind(dist[D.ZERO_Q], prefix, k1) == 209 <= CAP  # every row behind the prefix is the zero query's candidate
    assert np.signbit(rd[D.ZERO_Q]).all() and (rd[D.ZERO_Q] == 0).all()
    qf = _f32(q)
    with gpu_pkg.BruteForceIndex.from_u8(base, metric=1) as idx:
        idx.set_batch(B)
        with Moved(idx, (2, 0, 2)):
            ids, d, fl = dev_topk(idx, qf, 2, B, k)
        assert np.array_equal(d, rd) and (d[D.ZERO_Q] == 0).all()
        assert np.array_equal(ids, ri)
        assert np.array_equal(fl, D.tie_flags(rd)) and fl[D.ZERO_Q] == 1 and all(fl[j] == 1 for j in D.TIE_Q)
        with Moved(idx, (2, 0, 2)):
            hi, hd = idx.search_topk(qf, k)
        wi, wd = D.host_view(ri, rd, k)
        assert np.array_equal(hi, wi) and np.array_equal(hd, wd)
        idx.set_precision(1)
        ids1, d1, fl1 = dev_topk(idx, qf, 2, B, k)
        assert np.array_equal(ids, ids1) and _same_bits(d, d1) and np.array_equal(fl, fl1)
        h1 = idx.search_topk(qf, k)
        assert np.array_equal(hi, h1[0]) and _same_bits(hd, h1[1])


@pytest.mark.parametrize("r", [1, 17])
@pytest.mark.parametrize("dim", [96, 200])
@pytest.mark.parametrize("k", [50, 100, 128])
def test_wider_k(gpu_pkg, k, dim, r):
    n = P(gpu_pkg, k, dim) + 64 * 2 + r
    assert n - P(gpu_pkg, k, dim, n) <= CAP  # the rows behind the prefix cannot overflow a list
    base, q = _l2_data(52000 + 10 * k + dim + r, n, NQ, dim)
    _check_l2(gpu_pkg, base, q, k)


@pytest.mark.parametrize("behind", [1, 15, 16, 17, 63, 64, 65])
def test_filter_pass_ragged_block(gpu_pkg, behind):
    n = P(gpu_pkg, 16) + behind
    base, q = _l2_data(53000 + behind, n, NQ, 96)
    _check_l2(gpu_pkg, base, q, 16, host=False)


@pytest.mark.parametrize("n", [4097, 5009, 4159, None])
def test_prefix_is_the_whole_base(gpu_pkg, n):
    """n <= P: the store pass alone, its last block ragged by 1, 17 and 63 rows; None: n = P exactly"""
    n = n or P(gpu_pkg, 16)
    assert gpu_pkg.BruteForceIndex.wide_plan(n, 96, 16)[1] == n
    base, q = _l2_data(54000 + n, n, NQ, 96)
    _check_l2(gpu_pkg, base, q, 16, host=n != 5009)


def test_fewer_rows_than_k(gpu_pkg):
    """n = 20, k = 100: the slots past the rows are (-1, +inf)"""
    base, q = _l2_data(55000, 20, NQ, 96)
    base[19] = base[0]
    q[0] = base[0]
    _check_l2(gpu_pkg, base, q, 100)


@pytest.mark.parametrize("Bq", [1, 16, 17, 32])
def test_batch_widths_and_id_offset(gpu_pkg, Bq):
    """one and two query blocks per tile, full and ragged; ids carry the index's offset"""
    n = P(gpu_pkg, 16, 192) + 209
    base, q = _l2_data(56000, n, 64 + 8, 192)
    q = q[8:]  # (the queries that are rows of the end of the base come first: a batch of one has candidates behind the prefix)
    _check_l2(gpu_pkg, base, q[:2 * Bq], 16, nb=2, Bq=Bq, id_offset=1000, host=Bq == 17)


def _with_sqnorm(target, dim):
    """a byte vector whose squared norm is exactly `target`"""
    import math
    v = np.zeros(dim, dtype=np.uint8)
    left = target
    for i in range(dim):
        x = min(255, math.isqrt(left))
        v[i] = x
        left -= x * x
    assert left == 0 and sqnorm_max(v[None]) == target
    return v


@pytest.mark.parametrize("variant", ["half", "256", "negative", "norm"])
def test_refused_batches_are_answered_on_the_fp32_rows(gpu_pkg, variant):
    """Three batches in one device call, the middle one not a byte batch: every batch equals the reference, no flag is 2,
    and the counters move by (2, 1, 3).  `norm`: ||q||^2 + bmax = 2^24 runs on bytes, one more does not."""
    k = 16
    if variant == "norm":
        dim = 2048
        n = P(gpu_pkg, k, dim) + 209
        rng = np.random.default_rng(57000)
        base = rng.integers(0, 41, size=(n, dim)).astype(np.uint8)
        q = rng.integers(0, 41, size=(3 * B, dim)).astype(np.uint8)
        bmax = sqnorm_max(base)
        q[7] = _with_sqnorm(2 ** 24 - bmax, dim)              # batch 0: on the bound, a byte batch
        q[B + 5] = _with_sqnorm(2 ** 24 - bmax + 1, dim)      # batch 1: one above it
        qf = _f32(q)
    else:
        dim = 200
        n = P(gpu_pkg, k, dim) + 209
        base, q = _l2_data(57001, n, 3 * B, dim)
        qf = _f32(q)
        qf[B + 4, 10] = {"half": 0.5, "256": 256.0, "negative": -1.0}[variant]
    bf = _f32(base)
    # the fp32 chain of the kernels; on the integer queries every order gives the same bits
    oi1, od1 = oracle.search_bf(bf, qf, k + 1, dot_order="chain")
    dist = oracle.l2_matrix(qf, bf, dot_order="chain")
    ties = (od1[:, 1:] == od1[:, :-1]).any(1)
    wi = _ids_by_id_order(dist, oi1, od1, np.flatnonzero(~ties))
    with gpu_pkg.BruteForceIndex.from_u8(base) as idx:
        idx.set_batch(B)
        with Moved(idx, (2, 1, 3)):
            ids, d, fl = dev_topk(idx, qf, 3, B, k)
        assert not (fl == 2).any() and np.array_equal(fl != 0, ties)
        assert _same_bits(d, od1)
        assert np.array_equal(ids[~ties], wi[~ties])
        oi, od = oracle.search_bf(bf, qf, k, dot_order="chain")
        with Moved(idx, (2, 1, 3)):
            hi, hd = idx.search_topk(qf, k)
        assert np.array_equal(hi, oi) and np.array_equal(hd, od)
        idx.set_precision(1)
        ids1, d1, fl1 = dev_topk(idx, qf, 3, B, k)
        assert np.array_equal(ids, ids1) and _same_bits(d, d1) and np.array_equal(fl, fl1)


def test_overflow_takes_the_dense_fallback(gpu_pkg):
    """The 9000 rows behind the prefix are copies of one row and query 3 equals it: more than 8192 candidates, so the dense
    fallback answers that batch -- with the reference's result, for every query of it."""
    k, dim = 16, 40
    prefix = P(gpu_pkg, k, dim)
    n = prefix + 9000
    rng = np.random.default_rng(58000)
    base, q = u8_data(rng, n, NQ, dim)
    row = rng.integers(0, 256, size=dim).astype(np.uint8)
    base[prefix:] = row
    q[3] = row
    bf, qf = _f32(base), _f32(q)
    dist = oracle.l2_matrix(qf, bf)
    assert dist[3, :prefix].min() > 0
    cand = [_cand_behind(r, prefix, k + 1) for r in dist]
    assert cand[3] == 9000 > CAP and max(cand[B:]) <= CAP  # batch 0 overflows, batch 1 does not
    oi1, od1 = oracle.search_bf(bf, qf, k + 1)
    ties = (od1[:, 1:] == od1[:, :-1]).any(1)
    wi = _ids_by_id_order(dist, oi1, od1, np.flatnonzero(~ties))
    with gpu_pkg.BruteForceIndex.from_u8(base) as idx:
        idx.set_batch(B)
        with Moved(idx, (2, 0, 2)):
            ids, d, fl = dev_topk(idx, qf, 2, B, k)
        assert _same_bits(d, od1)
        assert (d[3] == 0).all() and np.array_equal(ids[3], prefix + np.arange(k + 1)) and fl[3] == 1
        assert not (fl == 2).any() and np.array_equal(fl != 0, ties)
        assert np.array_equal(ids[~ties], wi[~ties])
        oi, od = oracle.search_bf(bf, qf, k)
        hi, hd = idx.search_topk(qf, k)
        assert np.array_equal(hi, oi) and np.array_equal(hd, od)


def test_routes_left_alone(gpu_pkg):
    k = 16
    n = P(gpu_pkg, k, 96) + 209
    base, q = _l2_data(59000, n, NQ, 96)
    bf, qf = _f32(base), _f32(q)
    od1 = oracle.search_bf(bf, qf, k + 1)[1]
    # precision 1, and a k = 5 call
    with gpu_pkg.BruteForceIndex.from_u8(base) as idx:
        assert idx.wide_stats() == (0, 0, 0)  # zeros before the first wide call
        idx.set_precision(1)
        with Moved(idx, (0, 0, 2)):
            d = dev_topk(idx, qf, 2, B, k)[1]
        assert np.array_equal(d, od1)
        idx.set_precision(0)
        one = idx.one_stats()
        with Moved(idx, (0, 0, 0)):
            d5 = dev_topk(idx, qf, 2, B, 5)[1]
        assert np.array_equal(d5, oracle.search_bf(bf, qf, 6)[1]) and idx.one_stats() == one
        with Moved(idx, (2, 0, 2)):
            dev_topk(idx, qf, 2, B, k)
        assert idx.wide_stats(reset=True) == (2, 0, 4) and idx.wide_stats() == (0, 0, 0)
    # an index from float rows
    with gpu_pkg.BruteForceIndex(bf) as idx:
        with Moved(idx, (0, 0, 2)):
            d = dev_topk(idx, qf, 2, B, k)[1]
        assert np.array_equal(d, od1)
    # a from_u8 index whose byte copy was dropped: one row of 2048 x 255
    rng = np.random.default_rng(59001)
    n2 = P(gpu_pkg, k, 2048) + 209
    big = rng.integers(0, 41, size=(n2, 2048)).astype(np.uint8)
    big[1234] = 255
    q2 = _f32(rng.integers(0, 41, size=(NQ, 2048)).astype(np.uint8))
    with gpu_pkg.BruteForceIndex.from_u8(big) as idx:
        with Moved(idx, (0, 0, 2)):
            d = dev_topk(idx, q2, 2, B, k)[1]
        assert np.array_equal(d, oracle.search_bf(_f32(big), q2, k + 1, dot_order="chain")[1])
    # the specialised 128-d L2 index
    b128 = gpu_pkg.synth_sift(P(gpu_pkg, k, 128) + 209, seed=31).astype(np.uint8)
    q128 = gpu_pkg.synth_sift(NQ, seed=32)
    with gpu_pkg.BruteForceIndex.from_u8(b128) as idx:
        with Moved(idx, (0, 0, 2)):
            d = dev_topk(idx, q128, 2, B, k)[1]
        assert np.array_equal(d, oracle.search_bf(_f32(b128), q128, k + 1)[1])
        hi, hd = idx.search_topk(q128, k)
        oi, od = oracle.search_bf(_f32(b128), q128, k)
        assert np.array_equal(hi, oi) and np.array_equal(hd, od)


def test_interleaved_calls_share_the_scratch(gpu_pkg):
    """wide, k = 5, wide, a single-call short call on one index: each equals its reference"""
    import test_gpu_cancel as tc
    k = 50
    n = P(gpu_pkg, k, 320) + 209
    base, q = _l2_data(60000, n, 3 * 32, 320)
    bf, qf = _f32(base), _f32(q)
    w_wide = oracle.search_bf(bf, qf, k + 1)[1]
    w5 = oracle.search_bf(bf, qf, 6)[1]
    assert gpu_pkg.BruteForceIndex.one_plan_u8(n, 320, 256, 1, 12, 5)[0] == 3
    with gpu_pkg.BruteForceIndex.from_u8(base) as idx:
        with Moved(idx, (6, 0, 6)):
            a = dev_topk(idx, qf, 3, 32, k)[1]
            b = dev_topk(idx, qf, 3, 32, 5)[1]
            c = dev_topk(idx, qf, 3, 32, k)[1]
        one = idx.one_stats()[1]
        e = tc._bf_dev(idx, qf, 1, 12, 5, "one")[1]
        assert idx.one_stats()[1] == one + 1
        f = dev_topk(idx, qf, 1, 12, k)[1]
    assert np.array_equal(a, w_wide) and np.array_equal(c, w_wide) and np.array_equal(b, w5)
    assert np.array_equal(e, w5[:12]) and np.array_equal(f, w_wide[:12])


def test_toggle_keeps_the_fp32_launches(gpu_pkg, tmp_path):
    """A fresh process under VSEARCH_ND_WIDE_U8=0 returns the same outputs and counts no batch on the byte rows."""
    out = str(tmp_path / "fp32.npz")
    r = subprocess.run([sys.executable, os.path.abspath(child.__file__), ROOT, out],
                       env=dict(os.environ, VSEARCH_ND_WIDE_U8="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ND_WIDE_U8_CHILD_OK" in r.stdout, (r.stdout[-400:], r.stderr[-1500:])
    there = np.load(out)
    assert os.environ.get("VSEARCH_ND_WIDE_U8", "1") != "0"
    here = child.run(gpu_pkg)
    assert set(here) == set(there.files)
    calls = len(child.KS) * 2 * (child.NQ // child.B)  # a device call and a host call per k
    for key in here:
        if key.endswith("_stats"):
            assert tuple(there[key]) == (0, 0, calls), key
            refused = len(child.KS) * 2 if "refused" in key else 0
            assert tuple(here[key]) == (calls - refused, refused, calls), key
        elif key.endswith("d"):
            assert np.array_equal(here[key].view(np.int32), there[key].view(np.int32)), key
        else:
            assert np.array_equal(here[key], there[key]), key
    f = here["l2_65_refused_16_f"]
    assert not (f == 2).any()
