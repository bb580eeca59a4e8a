"""Byte-valued and other batches in ONE search_dev_multi launch on the specialised 128-d index, at device level.

Under precision 2 (or 0) a batch that holds a query value which is no integer in [0, 255] is skipped on the device: its
queries come back with flags == 2, ids -1 and distances +inf, and the caller reruns that batch alone under precision 1.
Every other batch of the launch is therefore exactly what the caller uses, and is checked here against exact integer
lists (mixed_batches_child.exact_lists: int64 distances from float64 products, ranked by (distance, id), k + 1 entries),
never against another GPU path.  The host calls cannot see a mistake there: they rerun the whole chunk on the fp32 rows
as soon as one flag of it is 2.

Data: rows are rng.integers(0, 256), queries clip(row + rng.integers(-3, 4), 0, 255); every fp32 quantity of either data
path is then an integer below 2^24, so the tolerance is "bit for bit" for the byte scan and for the fp32 rerun alike.
The bases are the smallest at which bf_launch takes another route: S = 3000 rows (no threshold exchange, no bound: the
big workgroup merge overlays the tile ring), M = 40000 (in-kernel threshold exchange), L = 65537 (launches of >= 4
batches are seeded and take the streaming scan_i8w_kernel, shorter ones scan_kernel with the exchange; ragged last
tile), and D = 100000 synth_sift rows of which 40000 are copies of one row, with two queries that overflow the streaming
scan's candidate buffers, so that the per-batch scan enqueued behind it produces the launch's result.

Launches (mixed_batches_child.MATRIX), each at (B, k) = (32, 5), (32, 15), (16, 5), (16, 15), (20, 5) -- the four
scan_kernel<NQH, KCAP, kModeTopK, 1> instantiations and a batch with padding columns; no combination was dropped:
    S, M, L   3 batches, skipped {0}, {1}, {2}, {0,1}, {0,2}, {0,1,2}
    L         8 batches, skipped {0}, {3}, {4}, {1,2}, {7}, {0,1,2,3}, {1,3,5,7}, all;  9 batches, skipped {8}, {4}
    D         5 batches, the two overflowing queries first in batch 1, skipped {0}, {2}
The plant is 7.5 in one element of one query of each skipped batch (row B - 1 and column 127 among the positions).  Each
launch is issued twice (identical bytes: the failure this module was written for differed from run to run) and followed
by a launch of byte-valued batches only (no flag 2: the verdict words are cleared per launch); one launch per base runs
under precision 0 as well.  rerun:X is the caller's side of the contract (plants 256.0 and -1.0: integers outside the
byte range, so the fp32 rerun of the planted queries stays exact), edges:L the values at which the verdict turns, in a
seeded launch (verdict from the seed launch) and an unseeded one (verdict from scan_kernel).

A query whose k + 1 nearest hold two equal distances is flagged 1 and only checked for a valid tie order, so the fixture
asserts on the reference alone, before any GPU call, that at most 1 % of the live queries of every launch are such.  The
two overflowing queries of D are tied by construction (40001 rows at one distance): they are asserted to BE tied and
left out of that count, which the other queries of D must meet.

One child process per setting of the VSEARCH_* knobs (they are read when the library loads); it runs every task of that
setting, and each test below looks up its own task in the child's report."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_batches_child as mb

pytestmark = pytest.mark.gpu

# Chosen on the reference alone: with this fixture's order of draws, seed 20272 gives S, M and L one tied query in all (on
# L, at k = 15), which keeps every launch under the cap and still has flag 1 checked in both directions; 20262 puts one
# tied query into a launch with 64 live ones (1.6 %).  Another seed has to pass the fixture's assertions the same way.
SEED = 20272
RUNS = {
    "default": ({}, ["matrix:S", "matrix:M", "matrix:L", "matrix:D", "rerun:S", "rerun:M", "rerun:L", "rerun:D", "edges:L"]),
    # seeded launches on the per-batch scan_kernel with tau0 given
    "no_streaming": ({"VSEARCH_STREAM": "0"}, ["matrix:L", "matrix:D", "edges:L"]),
    # two / six 32-query batches per pass: a dead batch on every position of a pass, and (12) a pass that is wholly dead
    "i8_wide_4": ({"VSEARCH_I8_WIDE": "4"}, ["matrix:L"]),
    "i8_wide_12": ({"VSEARCH_I8_WIDE": "12"}, ["matrix:L"]),
}


@pytest.fixture(scope="module")
def data_file(gpu_pkg, tmp_path_factory):
    """Bases, queries and the exact lists, computed once; the 99 % cap on the reference alone."""
    rng = np.random.default_rng(SEED)
    out = {}
    for X in "SML":
        n, nq = mb.ROWS[X], mb.NQ[X]
        base = rng.integers(0, 256, size=(n, 128)).astype(np.uint8)
        near = rng.integers(0, n, size=nq)
        q = np.clip(base[near].astype(np.int64) + rng.integers(-3, 4, size=(nq, 128)), 0, 255).astype(np.float32)
        out["base_" + X], out["q_" + X] = base, q
    base = gpu_pkg.synth_sift(mb.ROWS["D"], seed=74)
    base[20000:60000] = base[7]  # 40 000 copies of one row
    assert base.min() >= 0 and base.max() <= 255 and np.array_equal(base, np.rint(base))
    out["base_D"], out["q_D"] = base.astype(np.uint8), gpu_pkg.synth_sift(mb.NQ["D"], seed=75)
    out["ov_q"] = np.stack([base[7], base[7] + 1])
    for X in "SMLD":
        out["ri_" + X], out["rd_" + X] = mb.exact_lists(out["q_" + X], out["base_" + X])
    out["ov_ri"], out["ov_rd"] = mb.exact_lists(out["ov_q"], out["base_D"])
    for k in (5, 15):
        assert mb.tied(out["ov_rd"], k).all()
    for X in "SMLD":
        for B, k in mb.BK:
            rd = out["rd_" + X] if X != "D" else mb.d_lists(out["ri_D"], out["rd_D"], out["ov_ri"], out["ov_rd"], B)[1]
            for nb, skipped in mb.MATRIX[X]:
                mb.check_cap(rd, nb, B, k, skipped, (B, B + 1) if X == "D" else ())
    path = tmp_path_factory.mktemp("mixed_batches") / "data.npz"
    np.savez(path, **out)
    return str(path)


@pytest.fixture(scope="module")
def reports(data_file):
    """The report of a knob setting's child process, which is started once: {task: its TASK line}, and the output."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = {}

    def get(name):
        if name not in done:
            env, tasks = RUNS[name]
            e = dict(os.environ)
            e.update(env)
            r = subprocess.run([sys.executable, os.path.join(root, "tests", "mixed_batches_child.py"), root, data_file, ",".join(tasks)],
                               env=e, capture_output=True, text=True, timeout=300)
            lines = {ln.split()[1]: ln for ln in r.stdout.splitlines() if ln.startswith("TASK ")}
            done[name] = (r.returncode == 0 and "MIXED_BATCHES_DONE" in r.stdout, lines, r.stdout[-6000:], r.stderr[-1500:])
        return done[name]

    return get


@pytest.mark.parametrize("name,task", [(n, t) for n, (_, tasks) in RUNS.items() for t in tasks])
def test_mixed_batches_match_exact_lists(reports, name, task):
    finished, lines, out, err = reports(name)
    assert task in lines, (name, task, "the child did not reach the task", out[-1500:], err)
    assert lines[task] == f"TASK {task} OK", (name, [ln for ln in out.splitlines() if task.replace(":", "', '") in ln or ln.startswith("TASK " + task)])
    assert finished, (name, out[-1500:], err)
