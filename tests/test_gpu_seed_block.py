"""The seed on the int8 copy with a block of batches per workgroup (seed_block_kernel; VSEARCH_SEED_I8 unset or
2) against the seed with one batch per workgroup (VSEARCH_SEED_I8=1) and the CPU oracle.  The group minima are exact
integers, so the bounds, the candidates written and the results are the same numbers: ids, distance bits and flags are
compared byte for byte, there is no tolerance.

Shapes: the smallest shards a seeded launch takes (65 536 rows, and 65 536 + 37 with a partial last tile), byte valued,
k = 5, the int8 sweep forced at every launch size (VSEARCH_F32_FILTER_I8=2) so that its counter of written candidates pins
the bounds.  4, 5, 7, 8, 9 and 32 batches per call: full blocks, a block of one and short last blocks at blocks of 2 and
4 batches (sides nb2 / nb4 force each at every launch size; the default side is the library's own rule: one batch per
workgroup under 8 batches, blocks of 2 from 8, of 4 from 24); 32, 17 and 1 queries per batch.  Each side is one child process (seed_block_child.py), started once per session and shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import seed_block_child as ch  # noqa: E402

SIDES = {"default": {}, "per_batch": {"VSEARCH_SEED_I8": "1"}, "nb2": {"VSEARCH_SEED_NB": "2"}, "nb4": {"VSEARCH_SEED_NB": "4"}}
BLOCKED = ("default", "nb2", "nb4")
_RUNS, _ORACLE = {}, {}


def _side(tmp_path_factory, side):
    if side not in _RUNS:
        out = str(tmp_path_factory.mktemp("seed_block") / f"{side}.npz")
        env = dict(os.environ)
        for k in ("VSEARCH_F32_FILTER_I8", "VSEARCH_F32_FILTER_I8_RECHECK", "VSEARCH_F32_FILTER", "VSEARCH_F32F_WAVES", "VSEARCH_F32F_PRIO",
                  "VSEARCH_SEED_MIN", "VSEARCH_SEED_I8", "VSEARCH_SEED_NB", "VSEARCH_I8_WIDE"):
            env.pop(k, None)
        env["VSEARCH_F32_FILTER_I8"] = "2"
        env.update(SIDES[side])
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seed_block_child.py"), ROOT, out], env=env,
                           capture_output=True, text=True, timeout=300)
        print(f"--- side {side} ---\n{r.stdout[-6000:]}")
        assert r.returncode == 0, (side, r.returncode, r.stderr[-3000:])
        _RUNS[side] = dict(np.load(out))
    return _RUNS[side]


def _oracle(pkg, which, kind):
    """k + 2 nearest of the whole query set (or of the changed batch of a mixed set) by the CPU oracle, once per session."""
    import oracle
    if (which, kind) not in _ORACLE:
        base = ch.base_rows(pkg, which)
        if kind == "head":
            _ORACLE[(which, kind)] = oracle.search_bf(base, ch.query_set(pkg, "head", 32, 32), ch.K + 2, dot_order="chain")
        elif kind == "tail":  # the same queries backwards
            oi, od = _oracle(pkg, which, "head")
            _ORACLE[(which, kind)] = (oi[::-1], od[::-1])
        else:  # a mixed set: the head's results with the changed batch computed anew
            oi, od = (x.copy() for x in _oracle(pkg, which, "head"))
            b = ch.MIXED_ONE[0] if kind == "mixed_one" else ch.MIXED_LAST
            q = ch.query_set(pkg, kind, 32, 9)[32 * b: 32 * (b + 1)]
            oi[32 * b: 32 * (b + 1)], od[32 * b: 32 * (b + 1)] = oracle.search_bf(base, q, ch.K + 2, dot_order="chain")
            _ORACLE[(which, kind)] = (oi, od)
    return _ORACLE[(which, kind)]


def _same(a, b, key, what):
    for s in ("_i", "_d", "_f"):
        x, y = a[key + s], b[key + s]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key + s)


def _against_oracle(pkg, run, key, which, kind, B, nb):
    oi, od = _oracle(pkg, which, kind)
    n = nb * B
    gi, gd, f = run[key + "_i"], run[key + "_d"], run[key + "_f"]
    assert np.isin(f, (0, 1)).all(), (key, np.unique(f))
    oi, od = oi[:n], od[:n]
    assert np.array_equal(gd.view(np.uint32), od[:, :ch.K + 1].view(np.uint32)), (key, "distance bits differ from the oracle")
    tied = (np.diff(od[:, :ch.K + 1], axis=1) == 0).any(axis=1)
    assert np.array_equal(f == 1, tied), (key, "flag 1 is not 'an equal pair among the k + 1'")
    # ids are pinned where no two of the k + 1 distances are equal and the row behind the last one is farther
    plain = ~tied & (od[:, ch.K + 1] != od[:, ch.K])
    assert np.array_equal(gi[plain], oi[plain, :ch.K + 1]), (key, "ids differ from the oracle")
    return int(plain.sum())


PLAIN = [x for x in ch.LAUNCHES if x[4] == 1 and x[5] == "head" and x[0] != "ragged_long"]


@pytest.mark.gpu
@pytest.mark.parametrize("side", BLOCKED)
def test_block_and_batch_shapes_equal_the_per_batch_seed_and_the_oracle(gpu_pkg, tmp_path_factory, side):
    a, ref = _side(tmp_path_factory, side), _side(tmp_path_factory, "per_batch")
    plain = total = 0
    for key, which, B, nb, prec, kind in PLAIN:
        _same(a, ref, key, f"{side} against the per-batch seed")
        n = _against_oracle(gpu_pkg, a, key, which, kind, B, nb)
        plain, total = plain + n, total + nb * B
        sa, sr = [int(x) for x in a[key + "_i8"]], [int(x) for x in ref[key + "_i8"]]
        print(f"{key}: {n} of {nb * B} queries compared id for id; int8 stats {sa} per-batch {sr}")
        # on the int8 route, nothing handed over; equal bounds give equal candidate sets
        assert sa[0] == 1 and sa[1] == 0 and sa[2] == sa[3] > 0, key
        assert sa == sr, key
        assert a[key + "_bf16"].tolist() == ref[key + "_bf16"].tolist() and int(a[key + "_bf16"][1]) == 0, key
    assert plain >= total // 4, (plain, total)  # the id comparison has teeth: most queries have no tie among their k + 2


@pytest.mark.gpu
@pytest.mark.parametrize("side", BLOCKED)
@pytest.mark.parametrize("key", ["ragged_mixed_one", "ragged_mixed_last"])
def test_mixed_verdicts_in_one_block(gpu_pkg, tmp_path_factory, side, key):
    """A batch that is not byte valued inside a block (the second of a block; the last, a block of one): its minima come
    from the fp32 rows, the other batches' from the int8 body, and the group is answered by the bf16 sweep."""
    a, ref = _side(tmp_path_factory, side), _side(tmp_path_factory, "per_batch")
    _, which, B, nb, prec, kind = next(x for x in ch.LAUNCHES if x[0] == key)
    _same(a, ref, key, f"{side} against the per-batch seed")
    _against_oracle(gpu_pkg, a, key, which, kind, B, nb)
    sa, fa, fr = [int(x) for x in a[key + "_i8"]], [int(x) for x in a[key + "_bf16"]], [int(x) for x in ref[key + "_bf16"]]
    print(f"{key}: int8 stats {sa} bf16 stats {fa} per-batch {fr}")
    assert sa == [1, 1, 0, 0], key          # enqueued on the int8 route, handed to the bf16 sweep by the device
    assert sa == [int(x) for x in ref[key + "_i8"]], key
    assert fa == fr and fa[0] == 1 and fa[1] == 0 and fa[2] >= fa[3] > 0, key  # equal bounds: equal candidates written


@pytest.mark.gpu
@pytest.mark.parametrize("side", BLOCKED)
def test_precision_2_takes_the_same_bounds(gpu_pkg, tmp_path_factory, side):
    a, ref = _side(tmp_path_factory, side), _side(tmp_path_factory, "per_batch")
    key = "ragged_prec2"
    _, which, B, nb, prec, kind = next(x for x in ch.LAUNCHES if x[0] == key)
    _same(a, ref, key, f"{side} against the per-batch seed")
    _against_oracle(gpu_pkg, a, key, which, kind, B, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("side", BLOCKED)
def test_short_call_after_a_long_one_on_one_handle(gpu_pkg, tmp_path_factory, side):
    """32 batches, then 5 batches of other queries on the same handle: the short call's bounds are its own (stale minima of
    the long call would change the candidates written, or lose a neighbour)."""
    a, ref = _side(tmp_path_factory, side), _side(tmp_path_factory, "per_batch")
    for key in ("ragged_long", "ragged_short_after_long"):
        _, which, B, nb, prec, kind = next(x for x in ch.LAUNCHES if x[0] == key)
        _same(a, ref, key, f"{side} against the per-batch seed")
        _against_oracle(gpu_pkg, a, key, which, kind, B, nb)
        sa = [int(x) for x in a[key + "_i8"]]
        assert sa[0] == 1 and sa[1] == 0 and sa[2] == sa[3] > 0, key
        assert sa == [int(x) for x in ref[key + "_i8"]], key
