"""Byte-valued test data and the exact reference for inner-product brute force on uint8 rows (vs_bf_create_nd_u8_metric),
shared by test_nd_u8_ip_host.py and test_gpu_nd_u8_ip.py.

Data: nd_u8_data.u8_data (every squared norm under 2^23, the int8 extremes planted, duplicated rows at both ends) plus
planted edges, where the base and the query set are large enough to hold them:

  * query ZERO_Q is all zero: every product is 0, the k + 1 best are rows 0 .. k, all tied;
  * three all-zero rows (zero_rows(n));
  * queries ORTH_Q live on the first half of the columns and the rows orth_rows(n) on the second half: their products are
    exactly 0 (at dim 1 the "second half" is empty: those rows are zero rows);
  * for the queries TIE_Q the best row is copied to another position: their two best scores are equal.

Every value is >= 0, so a zero product is the smallest score there is: it shows in a top-k list only for the zero query or
on a base of at most k + 1 rows (small_orth_base).

Reference: the products in int64 (ip_int64), ranked by (-q.b, id).  Under the exactness rule (integers, ||q||^2 + ||b||^2
<= 2^24) every product is at most 2^23, so its float32 value is exact."""
import numpy as np

from nd_u8_data import sqnorm_max, u8_data

ZERO_Q = 5
ORTH_Q = (6, 7)
TIE_Q = (1, 2, 3)
MIN_ROWS = 64  # bases smaller than this carry no planted rows
MIN_QUERIES = 8


def zero_rows(n):
    return (n // 3, n // 3 + 1, n - 7)


def orth_rows(n):
    return (n // 2, n // 2 + 1, n // 2 + 5, n - 9)


def tie_rows(n):
    return tuple(n // 4 + j for j in range(len(TIE_Q)))


def _split(dim):
    return max(dim // 2, 1)  # queries ORTH_Q live on columns [0, split), rows orth_rows on [split, dim)


def ip_int64(q, base):
    """q.b for every (query, row), in int64."""
    q64 = np.asarray(q).astype(np.int64)
    out = np.empty((len(q64), len(base)), dtype=np.int64)
    for r0 in range(0, len(base), 8192):
        out[:, r0:r0 + 8192] = q64 @ np.asarray(base[r0:r0 + 8192]).astype(np.int64).T
    return out


def ip_data(rng, n, nq, dim):
    """(base uint8 [n, dim], queries uint8 [nq, dim]) with the planted edges."""
    base, q = u8_data(rng, n, nq, dim)
    s = _split(dim)
    if nq >= MIN_QUERIES:
        q[ZERO_Q] = 0
        for j in ORTH_Q:
            q[j, s:] = 0
            q[j, 0] = max(int(q[j, 0]), 3)
    if n >= MIN_ROWS:
        for r in zero_rows(n):
            base[r] = 0
        for r in orth_rows(n):
            base[r, :s] = 0
            if dim > 1:
                base[r, dim - 1] = max(int(base[r, dim - 1]), 2)
        if nq >= MIN_QUERIES:
            for j, r in zip(TIE_Q, tie_rows(n)):
                best = int(ip_int64(q[j:j + 1], base)[0].argmax())
                base[r] = base[best]
    assert sqnorm_max(base) < 2 ** 23 and sqnorm_max(q) < 2 ** 23
    return base, q


def small_orth_base(rng, dim, n=12):
    """(base [n, dim], queries [8, dim]): n <= 16 rows, so that k = 15 returns every row, the zero products included.  Rows
    1, 4 and n - 1 live on the second half of the columns, row 2 is zero; queries ORTH_Q live on the first half."""
    base, q = u8_data(rng, n, MIN_QUERIES, dim, dup=0.0)
    s = _split(dim)
    base[base == 0] = 1  # (no accidental zero products)
    q[q == 0] = 1
    q[ZERO_Q] = 0
    for j in ORTH_Q:
        q[j, s:] = 0
    for r in (1, 4, n - 1):
        base[r, :s] = 0
    base[2] = 0
    return base, q


def topk_ref(ip, k1, id_offset=0):
    """The k1 best rows per query by (-q.b, id): ids (int32, -1 in the slots past the rows) and the device scores
    -(float32)(q.b) (+inf in those slots; a zero product is -0.0)."""
    nq, n = ip.shape
    m = min(k1, n)
    ids = np.full((nq, k1), -1, dtype=np.int32)
    d = np.full((nq, k1), np.inf, dtype=np.float32)
    assert np.abs(ip).max() <= 2 ** 24
    for r in range(nq):
        kth = np.partition(ip[r], n - m)[n - m]
        cand = np.flatnonzero(ip[r] >= kth)  # every row at the m-th score: (score, id) then picks the right ones
        o = cand[np.lexsort((cand, -ip[r, cand]))[:m]]
        ids[r, :m] = o + id_offset
        d[r, :m] = -(ip[r, o].astype(np.float32))
    return ids, d


def host_view(ids, d, k):
    """What the host calls return for k: the first k columns, scores q.v descending (+inf where there is no row)."""
    i = ids[:, :k]
    return i, np.where(i >= 0, -d[:, :k], np.float32(np.inf)).astype(np.float32)


def tie_flags(d):
    """1 exactly where two finite neighbours of a list are equal."""
    return (np.isfinite(d[:, 1:]) & (d[:, 1:] == d[:, :-1])).any(1).astype(np.int32)
