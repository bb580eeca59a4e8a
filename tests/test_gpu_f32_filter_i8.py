"""The int8 prefilter sweep of the fp32 brute-force scan on a byte-valued shard (scan_f32f_i8_kernel), under
precision 1: ids, distance bits and flags bit for bit equal to the bf16 sweep alone (VSEARCH_F32_FILTER_I8=0), to
scan_f32s_kernel (VSEARCH_F32_FILTER=0) and to the CPU oracle -- the results are exact, there is no tolerance.

Shapes: the smallest seeded shard with a partial last unit (65 536 + 37 rows) and 131 072 rows; 4, 5, 9, 17 and 32
batches (1, 2, 4 and 8 column blocks per wave, both organisations); 32 and 7 queries per batch (padding queries); an id
offset; a mixed group (a value of 0.5 in one batch, of 256 in another: the device hands the group to the bf16 sweep);
queries forced onto near-ties (not byte valued: handed over as well); a shard of 64 distinct rows repeated (the lists
overflow and the fallback answers); an inner-product index (never on the route).  Each leg is one child process
(f32_filter_i8_child.py), started once per session and shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import f32_filter_i8_child as ch  # noqa: E402

# i8: the int8 sweep at every launch size, so that the small shard reaches its kernels of 1 and 2 column blocks per wave;
# rule: the library's own choice per launch size
LEGS = {"i8": {"VSEARCH_F32_FILTER_I8": "2"}, "rule": {}, "bf16": {"VSEARCH_F32_FILTER_I8": "0"}, "f32": {"VSEARCH_F32_FILTER": "0"}}
_RUNS, _ORACLE = {}, {}


def _leg(tmp_path_factory, leg):
    if leg not in _RUNS:
        out = str(tmp_path_factory.mktemp("f32f_i8") / f"{leg}.npz")
        env = dict(os.environ)
        for k in ("VSEARCH_F32_FILTER_I8", "VSEARCH_F32_FILTER", "VSEARCH_F32F_WAVES", "VSEARCH_F32F_PRIO", "VSEARCH_SEED_MIN", "VSEARCH_SEED_I8"):
            env.pop(k, None)
        env.update(LEGS[leg])
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "f32_filter_i8_child.py"), ROOT, out], env=env,
                           capture_output=True, text=True, timeout=600)
        print(f"--- leg {leg} ---\n{r.stdout[-6000:]}")
        assert r.returncode == 0, (leg, r.returncode, r.stderr[-3000:])
        _RUNS[leg] = dict(np.load(out))
    return _RUNS[leg]


def _oracle(which, kind):
    """k + 2 nearest of all the queries of a set by the CPU oracle (the fp32 chain order), once per session."""
    import oracle
    if (which, kind) not in _ORACLE:
        base = ch.base_rows(which)
        _ORACLE[(which, kind)] = oracle.search_bf(base, ch.query_set(kind, base, which), ch.K + 2, dot_order="chain")
    return _ORACLE[(which, kind)]


def _same(a, b, key, what):
    for s in ("_i", "_d", "_f"):
        x, y = a[key + s], b[key + s]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key + s)


def _against_oracle(run, key, which, kind, B, nb, id_offset):
    oi, od = _oracle(which, kind)
    n = nb * B
    gi, gd, f = run[key + "_i"], run[key + "_d"], run[key + "_f"]
    assert np.isin(f, (0, 1)).all(), (key, np.unique(f))
    oi, od = oi[:n], od[:n]
    assert np.array_equal(gd.view(np.uint32), od[:, :ch.K + 1].view(np.uint32)), (key, "distance bits differ from the oracle")
    tied = (np.diff(od[:, :ch.K + 1], axis=1) == 0).any(axis=1)
    assert np.array_equal(f == 1, tied), (key, "flag 1 is not 'an equal pair among the k + 1'")
    # ids are pinned where no two of the k + 1 distances are equal and the row behind the last one is farther (among
    # equal distances any order of the ids is valid, and the oracle's is not the library's)
    plain = ~tied & (od[:, ch.K + 1] != od[:, ch.K])
    assert np.array_equal(gi[plain], oi[plain, :ch.K + 1] + id_offset), (key, "ids differ from the oracle")
    return int(plain.sum())


@pytest.mark.gpu
def test_int8_sweep_equals_both_other_routes_and_the_oracle_bit_for_bit(gpu_pkg, tmp_path_factory):
    a, b, c = (_leg(tmp_path_factory, s) for s in ("i8", "bf16", "f32"))
    for key, which, metric, B, nb, id_offset, kind in ch.LAUNCHES:
        _same(a, b, key, "int8 sweep against the bf16 sweep")
        _same(a, c, key, "int8 sweep against scan_f32s_kernel")
        if metric == 0:
            plain = _against_oracle(a, key, which, kind, B, nb, id_offset)
            print(f"{key}: {plain} of {nb * B} queries without a tie compared id for id")
            if kind == "bytes":
                assert plain >= nb * B // 4, (key, plain)  # the check has teeth: the even queries' rows are not tied


@pytest.mark.gpu
def test_counters_of_a_byte_valued_group(gpu_pkg, tmp_path_factory):
    """One group on the int8 route, none handed over, no overflow, nothing written by the idle bf16 launch (filter_stats
    counts the candidates of both sweeps: all of them are the int8 sweep's); the int8 sweep
    keeps what the bf16 route keeps (both rechecks keep exactly the rows scan_f32s_kernel would), and writes no more."""
    a, b = (_leg(tmp_path_factory, s) for s in ("i8", "bf16"))
    for key in ch.ALL_BYTES:
        groups, handed, written, kept = (int(x) for x in a[key + "_i8"])
        launches, overflowed, w16, k16 = (int(x) for x in a[key + "_bf16"])
        ref = [int(x) for x in b[key + "_bf16"]]
        print(f"{key}: int8 (groups, handed over, written, kept) {(groups, handed, written, kept)}  idle bf16 {(launches, overflowed, w16, k16)}  bf16 route {ref}")
        assert groups == 1 and handed == 0, key
        assert int(a[key + "_plan"]) == 1, key
        assert launches == 1 and overflowed == 0 and w16 == written and k16 == kept, key
        assert 0 < kept <= written, key
        assert kept == ref[3] and ref[1] == 0, key
        assert written <= ref[2], key  # the integer test is exact; the bf16 test admits a widened set
        assert [int(x) for x in b[key + "_i8"]] == [0, 0, 0, 0], key  # the toggle: never on the route


@pytest.mark.gpu
def test_default_rule_takes_the_int8_sweep_where_it_was_measured_faster(gpu_pkg, tmp_path_factory):
    """Without the toggle: groups of more than 8 batches are on the route at every shard size, groups of 4 and 5 batches on
    these shards (4 and 8 units per workgroup, under the 24 of the rule) are not -- the counters agree with
    vs_bf_filter_i8_plan -- and the results are the same bytes either way."""
    a, r = (_leg(tmp_path_factory, s) for s in ("i8", "rule"))
    for key, which, metric, B, nb, id_offset, kind in ch.LAUNCHES:
        _same(a, r, key, "forced int8 sweep against the default rule")
        groups, plan = int(r[key + "_i8"][0]), int(r[key + "_plan"])
        print(f"{key}: plan {plan} groups {groups}")
        assert groups == plan, key
        assert plan == (1 if metric == 0 and nb > 8 else 0), key
        assert int(a[key + "_plan"]) == (1 if metric == 0 else 0), key


@pytest.mark.gpu
def test_group_with_a_batch_that_is_not_byte_valued_is_handed_to_the_bf16_sweep(gpu_pkg, tmp_path_factory):
    a, b = (_leg(tmp_path_factory, s) for s in ("i8", "bf16"))
    for key in ("a_mixed_nb9", "a_ties_nb4"):
        groups, handed, written, kept = (int(x) for x in a[key + "_i8"])
        st, ref = [int(x) for x in a[key + "_bf16"]], [int(x) for x in b[key + "_bf16"]]
        print(f"{key}: int8 {(groups, handed, written, kept)}  bf16 behind it {st}  bf16 route {ref}")
        assert (groups, handed, written, kept) == (1, 1, 0, 0), key
        assert st == ref and st[0] == 1 and st[1] == 0 and st[2] >= st[3] > 0, key


@pytest.mark.gpu
def test_overflow_takes_the_fallback(gpu_pkg, tmp_path_factory):
    """2048 copies of a row under every bound: the overflow word is raised by the int8 sweep and the fallback scan answers."""
    a = _leg(tmp_path_factory, "i8")
    key = "o_over_nb4"
    groups, handed, written, kept = (int(x) for x in a[key + "_i8"])
    launches, overflowed, w16, k16 = (int(x) for x in a[key + "_bf16"])
    print(f"{key}: int8 {(groups, handed, written, kept)}  bf16 {(launches, overflowed, w16, k16)}")
    assert groups == 1 and handed == 0 and overflowed == 1 and w16 == written
    assert (a[key + "_d"] == 0).all() and (a[key + "_f"] == 1).all()  # (the oracle comparison is in the first test)


@pytest.mark.gpu
def test_inner_product_index_stays_off_the_route(gpu_pkg, tmp_path_factory):
    a = _leg(tmp_path_factory, "i8")
    assert [int(x) for x in a["a_ip_nb4_i8"]] == [0, 0, 0, 0]
    assert int(a["a_ip_nb4_bf16"][0]) == 1 and int(a["a_ip_nb4_bf16"][2]) > 0
