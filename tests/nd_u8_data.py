"""Byte-valued test data for the uint8 creator (vs_bf_create_nd_u8), shared by test_nd_u8_host.py and test_gpu_nd_u8.py.

As tests/test_gpu_nd.py::_int_data: integer values in [0, hi) with 2 dim (hi - 1)^2 < 2^24, 5 % duplicated rows at both
ends of the base and queries that are duplicated rows, so that ties occur.  Every third row and query also carries the
values 255 and 0 in up to four columns: stored as (x - 128) they are the int8 extremes 127 and -128, which uniform values
under hi never reach above dim 129.  Every squared norm stays under 2^23, so ||q||^2 + ||b||^2 < 2^24 and the fp32
reference (oracle.search_bf) is exact on these inputs."""
import math

import numpy as np


def hi_of(dim):
    hi = min(int(math.isqrt((2 ** 23 - 1) // dim)) + 1, 256)
    assert 2 * dim * (hi - 1) ** 2 < 2 ** 24
    return hi


def _plant_extremes(rng, a):
    n, dim = a.shape
    c = min(4, dim)
    for i in range(0, n, 3):
        cols = rng.choice(dim, size=c, replace=False)
        a[i, cols[0::2]] = 255
        a[i, cols[1::2]] = 0


def sqnorm_max(a):
    return int((a.astype(np.int64) ** 2).sum(1).max())


def u8_data(rng, n, nq, dim, hi=None, dup=0.05):
    """(base uint8 [n, dim], queries uint8 [nq, dim])"""
    hi = hi or hi_of(dim)
    base = rng.integers(0, hi, size=(n, dim)).astype(np.uint8)
    q = rng.integers(0, hi, size=(nq, dim)).astype(np.uint8)
    _plant_extremes(rng, base)
    _plant_extremes(rng, q)
    m = int(n * dup / 2)
    if m > 0 and n >= 8 * m:
        # duplicates at both ends of the base, copied from rows of the middle
        src = rng.integers(2 * m, n - 2 * m, size=2 * m)
        base[:m] = base[src[:m]]
        base[n - m:] = base[src[m:]]
        for j in range(min(4, nq, 2 * m)):  # queries that ARE duplicated rows: their two best are tied at 0
            q[j] = base[src[j]]
    assert sqnorm_max(base) < 2 ** 23 and sqnorm_max(q) < 2 ** 23
    return base, q
