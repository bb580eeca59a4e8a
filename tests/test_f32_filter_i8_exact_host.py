"""The int8 prefilter sweep's entry is final (scan_f32f_i8_kernel): for a byte-valued pair the float the
sweep writes (vs_f32_filter_i8_dist: vs_kernels.h's filter_i8_dist, the function the kernel calls) has the bits of the
distance the fp32 recheck computed, and the recheck's keep is the sweep's exact test.  No GPU.

The recheck is emulated in float32 step by step: the dot product in RecheckF32's order (k = 16 c + 4 g + i: c, then i, then
g), ||q||^2 and ||b||^2 in the reference's order (eight lanes over x[8 i + j], then r0 + ... + r7: seed_qnorm_kernel,
row_sqnorm_kernel), d = fmaf(-2, dot, qn + bn).  numpy has no fmaf, so the test also asserts in int64 that every product
and every partial sum is an integer below 2^24: there a multiply-then-add is exact and equals the fmaf."""
import ctypes as C

import numpy as np
import pytest

LIM = 1 << 24
CHAIN = [16 * c + 4 * g + i for c in range(8) for i in range(4) for g in range(4)]


def _terms(q, b):
    """qterm, rterm, dot as the library defines them (include/vsearch.h, vs_f32_filter_i8_test), int64 [n]."""
    q, b = q.astype(np.int64), b.astype(np.int64)
    qterm = (q * q).sum(1) - 256 * (q - 128).sum(1) - 2 * 128 ** 3
    rterm = (b * b).sum(1) - 256 * (b - 128).sum(1)
    dot = ((q - 128) * (b - 128)).sum(1)
    assert np.array_equal(qterm + rterm - 2 * dot, ((q - b) ** 2).sum(1))
    return qterm, rterm, dot


def _sqnorm_f32(x):
    """||x||^2 in float32 in the kernels' order; asserts in int64 that every step is an integer below 2^24."""
    xf, xi = x.astype(np.float32), x.astype(np.int64)
    acc = np.zeros((len(x), 8), dtype=np.float32)
    acc_i = np.zeros((len(x), 8), dtype=np.int64)
    for i in range(16):
        prod = xf[:, 8 * i:8 * i + 8] * xf[:, 8 * i:8 * i + 8]
        assert prod.dtype == np.float32
        acc = acc + prod
        acc_i += xi[:, 8 * i:8 * i + 8] ** 2
        assert acc_i.max() < LIM and np.array_equal(acc.astype(np.int64), acc_i)
    s, s_i = acc[:, 0], acc_i[:, 0]
    for j in range(1, 8):
        s, s_i = s + acc[:, j], s_i + acc_i[:, j]
        assert s_i.max() < LIM and np.array_equal(s.astype(np.int64), s_i)
    assert s.dtype == np.float32
    return s


def _recheck_f32(q, b):
    """The fp32 recheck's distance (float32 [n]) for byte-valued pairs, step by step."""
    qf, bf = q.astype(np.float32), b.astype(np.float32)
    qi, bi = q.astype(np.int64), b.astype(np.int64)
    dot = np.zeros(len(q), dtype=np.float32)
    dot_i = np.zeros(len(q), dtype=np.int64)
    for k in CHAIN:
        prod = bf[:, k] * qf[:, k]
        dot = dot + prod
        dot_i += bi[:, k] * qi[:, k]
        assert (bi[:, k] * qi[:, k]).max() < LIM and dot_i.max() < LIM
        assert np.array_equal(prod.astype(np.int64), bi[:, k] * qi[:, k]) and np.array_equal(dot.astype(np.int64), dot_i)
    qn, bn = _sqnorm_f32(q), _sqnorm_f32(b)
    nsum = qn + bn
    nsum_i = (qi * qi).sum(1) + (bi * bi).sum(1)
    assert nsum_i.max() < LIM and np.array_equal(nsum.astype(np.int64), nsum_i)
    # fmaf(-2, dot, qn + bn): 2 dot is exact (a power of two), the difference an integer in [0, 2^24)
    d_i = nsum_i - 2 * dot_i
    assert d_i.min() >= 0 and d_i.max() < LIM
    d = nsum - np.float32(2.0) * dot
    assert d.dtype == np.float32 and np.array_equal(d.astype(np.int64), d_i)
    return d


@pytest.fixture(scope="module")
def i8(pkg):
    test, dist = pkg.lib().vs_f32_filter_i8_test, pkg.lib().vs_f32_filter_i8_dist
    out = (C.c_int32 * 3)()

    def exact(tau0, qterm, rterm, dot):  # plain Python numbers: the calls are the test's running time
        test(tau0, qterm, rterm, dot, out)
        return out[2] != 0

    return dist, exact


def _taus(d):
    """The bounds around each distance of d (float32 [n]): d, its neighbours, d +- 0.5, +-inf, NaN."""
    inf = np.float32(np.inf)
    full = lambda v: np.full(d.shape, v, dtype=np.float32)
    ts = [d, np.nextafter(d, inf), np.nextafter(d, -inf), d + np.float32(0.5), d - np.float32(0.5), full(inf), full(-inf), full(np.nan)]
    assert all(t.dtype == np.float32 for t in ts)
    return ts


def _check_pairs(i8, q, b):
    dist, exact = i8
    qterm, rterm, dot = _terms(q, b)
    want = _recheck_f32(q, b)
    qterm, rterm, dot = qterm.tolist(), rterm.tolist(), dot.tolist()
    got = np.array([dist(qterm[n], rterm[n], dot[n]) for n in range(len(q))], dtype=np.float32)
    assert got.tobytes() == want.tobytes(), "the sweep's float differs from the recheck's in some bit"
    taus = _taus(want)                                          # [8][n] float32
    keeps = [(want < t).tolist() for t in taus]                 # the recheck's keep: d < tau0 implies its hot test (stream_l2_thr)
    taus = [t.astype(np.float64).tolist() for t in taus]        # (exact: c_float gets the same float32 back)
    for n in range(len(q)):
        for t, keep in zip(taus, keeps):
            assert exact(t[n], qterm[n], rterm[n], dot[n]) == keep[n], (n, float(want[n]), t[n])
    return len(taus) * len(q)


def test_random_byte_pairs(i8):
    rng = np.random.default_rng(1101)
    n = 100_000
    q = rng.integers(0, 256, (n, 128))
    b = rng.integers(0, 256, (n, 128))
    # a share of SIFT-like small values, of near pairs (small distances of either parity) and of equal pairs
    q[: n // 4] = np.minimum(rng.gamma(1.2, 24.0, (n // 4, 128)), 255).astype(np.int64)
    b[: n // 4] = np.minimum(rng.gamma(1.2, 24.0, (n // 4, 128)), 255).astype(np.int64)
    near = slice(n // 4, n // 2)
    b[near] = np.clip(q[near] + (rng.random((n // 4, 128)) < 0.05) * rng.integers(-2, 3, (n // 4, 128)), 0, 255)
    b[n // 2: n // 2 + 100] = q[n // 2: n // 2 + 100]
    n_tau = _check_pairs(i8, q, b)
    print(f"{n} pairs bit for bit, {n_tau} bounds")


def test_extremes(i8):
    lo, hi = np.zeros(128, dtype=np.int64), np.full(128, 255, dtype=np.int64)
    mix = np.where(np.arange(128) % 2 == 0, 0, 255)
    one = lo.copy()
    one[77] = 1           # a single differing coordinate: d = 1, odd row term against lo
    two = hi.copy()
    two[5] = 253          # d = 4 against hi
    mid = np.full(128, 128, dtype=np.int64)
    mid1 = mid.copy()
    mid1[0] = 129
    pairs = [(lo, hi), (hi, lo), (hi, hi), (lo, lo), (lo, one), (one, lo), (hi, two), (mix, 255 - mix), (mix, mix), (mid, mid1), (mid1, mid),
             (one, hi), (two, lo)]
    q = np.stack([p[0] for p in pairs])
    b = np.stack([p[1] for p in pairs])
    qterm, rterm, dot = _terms(q, b)
    d = qterm + rterm - 2 * dot
    assert d[0] == 128 * 255 ** 2 == 8_323_200 and d[2] == 0
    assert (hi * hi).sum() * 2 == 16_646_400 < LIM
    assert {int(x) & 1 for x in rterm} == {0, 1}  # odd and even row terms
    _check_pairs(i8, q, b)
    dist, _ = i8
    zero = np.float32(dist(int(qterm[2]), int(rterm[2]), int(dot[2])))
    assert zero.tobytes() == np.float32(0.0).tobytes()  # +0.0, not -0.0
