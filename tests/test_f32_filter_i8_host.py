"""The integer test of the int8 prefilter sweep (scan_f32f_i8_kernel) as the library computes it
(vs_f32_filter_i8_test: vs_kernels.h's filter_i8_thr / filter_i8_c0 / filter_i8_hot / filter_i8_exact, the functions the
kernel calls).  No GPU.

With acc = sum (q - 128)(b - 128), qterm = ||q||^2 - 256 sum(q - 128) - 2 * 128^3 and rterm = ||b||^2 - 256 sum(b - 128) the
distance is d = qterm + rterm - 2 acc.  The sweep must admit every pair with d < tau0 (the fp32 recheck decides the rest);
its exact test must admit nothing else."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def i8_test(pkg):
    fn = pkg.lib().vs_f32_filter_i8_test

    def run(tau0, qterm, rterm, dot):
        out = (C.c_int32 * 3)()
        fn(C.c_float(tau0), int(qterm), int(rterm), int(dot), out)
        return int(out[0]), bool(out[1]), bool(out[2])

    return run


def _terms(q, b):
    q, b = q.astype(np.int64), b.astype(np.int64)
    qterm = (q * q).sum() - 256 * (q - 128).sum() - 2 * 128 ** 3
    rterm = (b * b).sum() - 256 * (b - 128).sum()
    dot = ((q - 128) * (b - 128)).sum()
    d = ((q - b) ** 2).sum()
    assert qterm + rterm - 2 * dot == d
    return int(qterm), int(rterm), int(dot), int(d)


def _next_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def test_threshold_and_the_rh_ro_split(i8_test):
    """thr = qterm - ceil(tau0); the hot test compares dot - (rterm >> 1) with floor(thr / 2) (an odd thr lowered by one), the
    exact test is d < tau0 -- for even and odd row terms, even and odd thr, negative values included."""
    for qterm in (-7, -2, 0, 5, 1234567):
        for rterm in (-9, -4, 0, 3, 8, 7654321):
            for tau in (0.0, 0.5, 1.0, 17.0, _next_up(17.0), 18.0, 1e6):
                thr_want = qterm - int(np.ceil(np.float32(tau)))
                for dot in range(-6, 7):
                    dot += (rterm + thr_want) // 2  # around the boundary
                    thr, hot, exact = i8_test(tau, qterm, rterm, dot)
                    d = qterm + rterm - 2 * dot
                    assert thr == thr_want
                    assert exact == (d < np.float32(tau)), (qterm, rterm, tau, dot)
                    assert hot == (dot - (rterm >> 1) > (thr >> 1))
                    if exact:
                        assert hot, (qterm, rterm, tau, dot)
                    # the hot test is wider by at most the odd-thr case: 2 A - ro = thr with ro = 1
                    if hot and not exact:
                        assert thr & 1 and rterm & 1 and 2 * (dot - (rterm >> 1)) - 1 == thr, (qterm, rterm, tau, dot)


def test_every_pair_under_the_bound_passes(i8_test):
    rng = np.random.default_rng(31)
    q = rng.integers(0, 256, (24, 128))
    b = rng.integers(0, 256, (160, 128))
    b[:24] = np.clip(q + rng.integers(-2, 3, q.shape), 0, 255)  # near rows: small distances of either parity
    n_under = n_hot_only = 0
    for i in range(len(q)):
        ds = ((q[i][None, :] - b) ** 2).sum(1)
        for tau in (_next_up(np.sort(ds)[5]), float(np.sort(ds)[5]), float(np.median(ds)) + 0.5):
            for j in range(len(b)):
                qterm, rterm, dot, d = _terms(q[i], b[j])
                _, hot, exact = i8_test(tau, qterm, rterm, dot)
                assert exact == (d < tau)
                assert hot or not exact
                n_under += exact
                n_hot_only += hot and not exact
    print(f"{n_under} pairs under their bound, {n_hot_only} admitted by the hot test alone")
    assert n_under > 1000


def test_extremes(i8_test):
    """||q||^2 + ||b||^2 just under 2^24 (all 255 against all 0 and all 255), values 0 and 255, tau0 = next_up of an exact
    distance and the distance itself, and the bounds that admit everything / nothing."""
    lo, hi = np.zeros(128, dtype=np.int64), np.full(128, 255, dtype=np.int64)
    mix = np.where(np.arange(128) % 2 == 0, 0, 255)
    assert 2 * 128 * 255 ** 2 < 1 << 24
    for q in (lo, hi, mix):
        for b in (lo, hi, mix, 255 - mix):
            qterm, rterm, dot, d = _terms(q, b)
            assert 0 <= d == float(np.float32(d)) < 1 << 24
            _, hot, exact = i8_test(_next_up(d), qterm, rterm, dot)
            assert hot and exact, (d,)
            _, hot, exact = i8_test(float(d), qterm, rterm, dot)
            assert not exact
            assert i8_test(float("inf"), qterm, rterm, dot)[1:] == (True, True)
            assert i8_test(float("-inf"), qterm, rterm, dot)[1:] == (False, False)
            assert i8_test(float("nan"), qterm, rterm, dot)[1:] == (False, False)
            assert i8_test(3e9, qterm, rterm, dot)[1:] == (True, True)
