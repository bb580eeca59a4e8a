"""Host-side checks of the UFIXED_POINT_8 runner's top-k up to k = 128 (vs_q8_search_topk*, vs_q8_topk_scores_dev,
vs_q8_wide_plan): the numpy reference against the oracle, the preconditions of the crafted matrices the GPU tests use,
the plan, the symbols and the calls that must refuse without a device.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import q8_wide_ref as ref
from q8_wide_ref import CHUNK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vs_q8_search_topk_dev", "vs_q8_search_topk", "vs_q8_topk_scores_dev", "vs_q8_wide_plan")


def _same_as_oracle(mat, k):
    wi, wt = ref.topk_ref(mat, k)
    oi, ot = oracle.q8_topk(mat, k)
    assert np.array_equal(wi, oi) and np.array_equal(wt, ot)
    return wi, wt


@pytest.mark.parametrize("k", [17, 128])
def test_reference_is_the_oracle(k):
    """vo_q8_topk visits rows in ascending order and replaces only on strictly larger: the lexsort order."""
    _same_as_oracle(ref.random_bytes(3001, 5), k)
    two = (ref.random_bytes(3001, 5) & 1) * 200  # two levels
    _same_as_oracle(two.astype(np.uint8), k)
    for v in (0, 7, 255):
        wi, _ = _same_as_oracle(ref.constant(500, 2, v), k)
        assert np.array_equal(wi[0], np.arange(k))
    for n in (1, 3, 16):  # n < k: the tail is (-1, 0), zero-score rows are entries
        wi, wt = _same_as_oracle(ref.random_bytes(n, 3), k)
        assert (wi[:, n:] == -1).all() and (wt[:, n:] == 0).all() and (np.sort(wi[:, :n], axis=1) == np.arange(n)).all()
        wi, _ = _same_as_oracle(ref.constant(n, 3, 0), k)
        assert np.array_equal(wi[0, :n], np.arange(n))
    wi, _ = ref.topk_ref(ref.constant(40, 1, 9), 17, id_offset=1000)
    assert np.array_equal(wi[0], 1000 + np.arange(17))


def test_narrow_and_rare_preconditions():
    m = ref.narrow_range(70001, 4)
    assert m.min() == 200 and m.max() == 203 and ((m == 203).sum(axis=1) > 10000).all()
    wi, wt = ref.topk_ref(m, 100)
    assert (wt == 203).all()
    for b in range(4):
        assert np.array_equal(wi[b], np.flatnonzero(m[b] == 203)[:100])
    m = ref.rare_top(70001, 4)
    assert ((m > 0).sum(axis=1) == 37).all() and m.max() == 1  # fewer than k rows above zero
    for b in range(4):
        assert len(set(np.flatnonzero(m[b]) // CHUNK)) == 5  # in every chunk
    wi, wt = ref.topk_ref(m, 100)
    assert (wt[:, :37] == 1).all() and (wt[:, 37:] == 0).all()
    for b in range(4):
        zeros = np.flatnonzero(m[b] == 0)[:63]
        assert np.array_equal(wi[b, 37:], zeros)


def test_two_tile_precondition():
    n = 65 * CHUNK + 5
    m = ref.rare_top(n, 2, ones=70)
    assert ref.plan_ref(n)[0] == 66 and ((m > 0).sum(axis=1) == 70).all()
    for b in range(2):
        ones = np.flatnonzero(m[b])
        assert len(set(ones // CHUNK)) == 66 and ones[-1] >= 65 * CHUNK  # a one in every chunk, the last past chunk 63


@pytest.mark.parametrize("n", [16383, 16384, 16385, 32768, 32769])
def test_boundary_preconditions(n):
    m, ks = ref.boundaries(n)
    assert set(ks) == {"whole_bin"} | ({"last_of_chunk0"} if n >= CHUNK else set()) | ({"first_of_chunk1"} if n > CHUNK else set())
    for b in range(2):
        nines = np.flatnonzero(m[b] == 9)
        assert len(nines) >= 2 and m[b].max() == 9
        for bd in range(CHUNK, n, CHUNK):  # value 9 and the run of 7 on both sides of every boundary inside the matrix
            assert (nines < bd).any() and (m[b, bd - 20:bd] == 7).all() and m[b, bd] == 7
            assert n <= bd + 20 or (nines >= bd).any()
        for case, k in ks.items():
            assert 17 <= k <= 128
            wi, wt = ref.topk_ref(m[b:b + 1], k)
            assert wt[0, k - 1] == 7 and (wt[0] >= 7).all()
            if case == "last_of_chunk0":
                assert wi[0, k - 1] == CHUNK - 1
            elif case == "first_of_chunk1":
                assert wi[0, k - 1] == CHUNK
            else:
                assert (m[b] >= 7).sum() == k


def test_inner_run_preconditions():
    m = ref.inner_runs()
    assert m.shape[1] <= CHUNK
    ends = {}
    for k in ref.INNER_KS:
        wi, wt = ref.topk_ref(m, k)
        assert (wt[0] == 7).all() and wt[1, min(k, 92) - 1] == 7  # k ends inside a run of the cut value (92 rows in query 1)
        ends[k] = wi[:, k - 1]
    assert ends[68][0] == 127 and ends[69][0] == 128 and 60 <= ends[17][0] <= 200 and ends[128][0] <= 200
    assert ends[77][1] == 4095 and ends[78][1] == 4096 and 4096 < ends[80][1] <= 4110


def test_level_preconditions():
    m = ref.levels_cycle(40000, 3)
    for b in range(3):
        assert len(np.unique(m[b])) == 256
    m, rows = ref.spread_top()
    assert len(rows) == 128 and (rows < m.shape[1]).all()
    places = {(r // CHUNK, (r % CHUNK) // 64) for r in rows}
    assert len(places) == 128 and len({c for c, _ in places}) == 5
    wi, wt = ref.topk_ref(m, 128)
    assert np.array_equal(wt[0], np.arange(255, 127, -1)) and np.array_equal(wi[0], rows[::-1])


def test_padded_layout():
    p = ref.padded(ref.random_bytes(70001, 2))
    assert p.shape == (2, 70016) and (p[:, 70001:] == 255).all()


def test_symbols_are_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "vsearch.h")).read()
    declared = set(re.findall(r"VS_API\s+[\w\s\*]+?\b(vs_\w+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared
        assert name in pkg.exported_symbols()
        assert hasattr(pkg.lib(), name)
    for name in ("search_topk", "search_topk_dev", "topk_scores_dev"):
        assert hasattr(pkg.Q8Runner, name)
    assert hasattr(pkg, "q8_wide_plan")
    hpp = open(os.path.join(ROOT, "include", "vsearch.hpp")).read()
    assert "vs_q8_search_topk(" in hpp


def test_null_handle_is_refused_without_a_device(pkg):
    L = pkg.lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    for k in (5, 100, 129):  # the handle is checked before k
        assert L.vs_q8_search_topk_dev(None, p, 1, 4, k, p, p, None) == -1
        assert L.vs_q8_search_topk(None, p, 4, k, p, p) == -1
        assert L.vs_q8_topk_scores_dev(None, p, 64, 4, k, p, p, None) == -1


@pytest.mark.parametrize("n_rows,chunks", [(1, 1), (16384, 1), (16385, 2), (1000003, 62)])
def test_plan_values(pkg, n_rows, chunks):
    for k in (17, 100, 128):
        got = pkg.q8_wide_plan(n_rows, k)
        assert got == ref.plan_ref(n_rows) and got[:2] == (chunks, 16384)
    assert pkg.q8_wide_plan(1, 17)[2] == 32768 + 128 + 128 + 20480
    assert pkg.q8_wide_plan(1000003, 100)[2] == 62 * 32768 + 128 + 62 * 128 + 20480


@pytest.mark.parametrize("n_rows,k", [(1000, 16), (1000, 129), (1000, 0), (0, 100), (-5, 100)])
def test_plan_refuses(pkg, n_rows, k):
    out = (C.c_int64 * 3)(7, 7, 7)
    assert pkg.lib().vs_q8_wide_plan(n_rows, k, out) == -1
    assert list(out) == [7, 7, 7]
    assert pkg.lib().vs_q8_wide_plan(1000, 100, None) == -1
    with pytest.raises(pkg.VSearchError) as e:
        pkg.q8_wide_plan(n_rows, k)
    assert e.value.status == -1
