"""Reference and crafted score matrices for the UFIXED_POINT_8 runner's top-k up to k = 128 (vs_q8_search_topk*,
vs_q8_topk_scores_dev).  The reference is numpy: np.lexsort((ids, -scores))[:k] per query, padded with (-1, 0): score
descending, equal scores in ascending row number.  Every generator is seeded, computed once and returned read-only."""
import functools

import numpy as np

CHUNK = 16384  # rows per chunk of the counting select (vs_q8_wide_plan's out[1])
PAD = 255      # what the tests put into the bytes between n and ld: a counted padding byte would win every ranking


def topk_ref(scores, k, id_offset=0):
    scores = np.asarray(scores, dtype=np.uint8)
    B, n = scores.shape
    ids = np.full((B, k), -1, dtype=np.int32)
    top = np.zeros((B, k), dtype=np.uint8)
    rows = np.arange(n)
    for b in range(B):
        order = np.lexsort((rows, -scores[b].astype(np.int64)))[:k]
        ids[b, :len(order)] = order + id_offset
        top[b, :len(order)] = scores[b, order]
    return ids, top


def ld_of(n):
    return (n + 63) // 64 * 64


def padded(mat):
    """[B, ld] with ld = n rounded up to 64 and PAD behind the rows."""
    B, n = mat.shape
    out = np.full((B, ld_of(n)), PAD, dtype=np.uint8)
    out[:, :n] = mat
    return out


def plan_ref(n_rows):
    c = -(-n_rows // CHUNK)
    return c, CHUNK, 32 * c * 1024 + 32 * 4 + 32 * c * 4 + 32 * 128 * 5


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def random_bytes(n, B, seed=0):
    return _ro(np.random.default_rng(1000 * n + B + seed).integers(0, 256, size=(B, n), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def narrow_range(n, B):
    """Values 200 .. 203 at random: the cut bin (203) holds about n / 4 rows."""
    return _ro(np.random.default_rng(203).integers(200, 204, size=(B, n), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def rare_top(n, B, ones=37):
    """All 0 except `ones` rows of value 1 per query, at least one in every chunk."""
    rng = np.random.default_rng(37)
    chunks = -(-n // CHUNK)
    assert ones >= chunks
    m = np.zeros((B, n), dtype=np.uint8)
    for b in range(B):
        rows = {int(rng.integers(c * CHUNK, min(n, (c + 1) * CHUNK))) for c in range(chunks)}
        while len(rows) < ones:
            rows.add(int(rng.integers(0, n)))
        m[b, sorted(rows)] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def constant(n, B, value):
    return _ro(np.full((B, n), value, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def boundaries(n):
    """Background 5; around every multiple bd of CHUNK up to n (rows past n - 1 dropped): value 7 on rows
    [bd - 20, bd + 20), value 9 on rows bd - 22, bd - 21, bd + 20, bd + 21.  Query 1 also has values below the
    background sprinkled in.  Returns (matrix [2, n], {case: k}):
      'last_of_chunk0'  the last taken row of bin 7 is row CHUNK - 1   (n >= CHUNK)
      'first_of_chunk1' ... is row CHUNK                               (n > CHUNK)
      'whole_bin'       ge[7] == k: every row of bin 7, no row of bin 5"""
    m = np.full((2, n), 5, dtype=np.uint8)
    m[1, np.random.default_rng(n).choice(n, n // 3, replace=False)] = 3
    for bd in range(CHUNK, n + CHUNK, CHUNK):
        for r in range(bd - 20, bd + 20):
            if r < n:
                m[:, r] = 7
        for r in (bd - 22, bd - 21, bd + 20, bd + 21):
            if r < n:
                m[:, r] = 9
    nines = int((m[0] == 9).sum())
    sevens = np.flatnonzero(m[0] == 7)
    ks = {"whole_bin": nines + len(sevens)}
    if n >= CHUNK:
        ks["last_of_chunk0"] = nines + int(np.searchsorted(sevens, CHUNK - 1)) + 1
    if n > CHUNK:
        ks["first_of_chunk1"] = nines + int(np.searchsorted(sevens, CHUNK)) + 1
    return _ro(m), ks


INNER_KS = (17, 68, 69, 77, 78, 80, 128)


@functools.lru_cache(maxsize=None)
def inner_runs(n=5000):
    """One chunk, background 5, cut value 7.  Query 0: rows 60 .. 200 and 4090 .. 4110 (the k of INNER_KS end inside the
    first run: k = 68 takes row 127, the last of thread 1, k = 69 row 128).  Query 1: every other row of 60 .. 200 (71 rows)
    and 4090 .. 4110: k = 77 ends on row 4095, the last of wave 0, k = 78 on row 4096, k = 80 inside the run."""
    m = np.full((2, n), 5, dtype=np.uint8)
    m[0, 60:201] = 7
    m[0, 4090:4111] = 7
    m[1, 60:201:2] = 7
    m[1, 4090:4111] = 7
    return _ro(m)


@functools.lru_cache(maxsize=None)
def levels_cycle(n, B):
    """score = 255 - (r mod 256): all 256 levels, n / 256 rows each; query b rotated by 37 b."""
    r = np.arange(n)
    return _ro(np.stack([(255 - ((r + 37 * b) % 256)).astype(np.uint8) for b in range(B)]))


@functools.lru_cache(maxsize=None)
def spread_top(n=70001):
    """The top 128 are the 128 values 128 .. 255, one each, in 128 different (chunk, thread) places; the rest is below 101.
    Returns (matrix [2, n], the rows of the values 128 .. 255 in value order)."""
    rng = np.random.default_rng(128)
    m = rng.integers(0, 101, size=(2, n), dtype=np.uint8)
    chunks = -(-n // CHUNK)
    rows = []
    for i in range(128):
        c = i % chunks
        width = min(CHUNK, n - c * CHUNK) // 64  # whole threads of the chunk
        rows.append(c * CHUNK + ((7 * i + 1) % width) * 64 + (i * 11) % 64)
    rows = np.array(rows)
    m[:, rows] = np.arange(128, 256, dtype=np.uint8)
    return _ro(m), rows
