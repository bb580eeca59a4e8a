"""The int8 prefilter sweep bins its entries as they stand (scan_f32f_i8_kernel): for a byte-valued pair the
integer distance is the fp32 distance.  Ids, distance bits and flags must be the same bytes with the entries final (the
default), with every entry recomputed from the fp32 rows (VSEARCH_F32_FILTER_I8_RECHECK=1) and from scan_f32s_kernel
(VSEARCH_F32_FILTER=0) -- there is no tolerance.

Shapes: the smallest seeded shard with a partial last unit (65 536 + 37 rows), the int8 sweep forced at every launch size
(VSEARCH_F32_FILTER_I8=2); 4, 9 and 32 batches (1, 4 and 8 column blocks per wave, both wave organisations); 32 and 7
queries per batch; an id offset.  Random SIFT-range bytes with a row of all 0 and a row of all 255, and a query of all 0
and one of all 255 in every batch.  Each side is one child process (f32_filter_i8_exact_child.py), started once per
session and shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import f32_filter_i8_exact_child as ch  # noqa: E402

SIDES = {
    "final": {"VSEARCH_F32_FILTER_I8": "2"},
    "recheck": {"VSEARCH_F32_FILTER_I8": "2", "VSEARCH_F32_FILTER_I8_RECHECK": "1"},
    "f32": {"VSEARCH_F32_FILTER": "0"},
}
_RUNS = {}


def _side(tmp_path_factory, side):
    if side not in _RUNS:
        out = str(tmp_path_factory.mktemp("f32f_i8_exact") / f"{side}.npz")
        env = dict(os.environ)
        for k in ("VSEARCH_F32_FILTER_I8", "VSEARCH_F32_FILTER_I8_RECHECK", "VSEARCH_F32_FILTER", "VSEARCH_F32F_WAVES", "VSEARCH_F32F_PRIO",
                  "VSEARCH_SEED_MIN", "VSEARCH_SEED_I8"):
            env.pop(k, None)
        env.update(SIDES[side])
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "f32_filter_i8_exact_child.py"), ROOT, out], env=env,
                           capture_output=True, text=True, timeout=300)
        print(f"--- side {side} ---\n{r.stdout[-4000:]}")
        assert r.returncode == 0, (side, r.returncode, r.stderr[-3000:])
        _RUNS[side] = dict(np.load(out))
    return _RUNS[side]


@pytest.mark.gpu
def test_final_entries_equal_the_recheck_and_the_fp32_scan_byte_for_byte(gpu_pkg, tmp_path_factory):
    a, b, c = (_side(tmp_path_factory, s) for s in ("final", "recheck", "f32"))
    for key, B, nb, id_offset in ch.LAUNCHES:
        for s in ("_i", "_d", "_f"):
            x = a[key + s]
            for other, what in ((b, "recheck"), (c, "scan_f32s_kernel")):
                y = other[key + s]
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key + s)
        assert np.isin(a[key + "_f"], (0, 1)).all(), key
        assert np.isfinite(a[key + "_d"]).all() and (a[key + "_i"] >= id_offset).all(), key


@pytest.mark.gpu
def test_counters_written_equals_kept_on_both_sides(gpu_pkg, tmp_path_factory):
    a, b = (_side(tmp_path_factory, s) for s in ("final", "recheck"))
    for key, B, nb, id_offset in ch.LAUNCHES:
        sa, sb = [int(x) for x in a[key + "_i8"]], [int(x) for x in b[key + "_i8"]]
        fa, fb = [int(x) for x in a[key + "_bf16"]], [int(x) for x in b[key + "_bf16"]]
        print(f"{key}: final {sa} {fa}  recheck {sb} {fb}")
        for groups, handed, written, kept in (sa, sb):
            assert groups == 1 and handed == 0, key
            assert written == kept > 0, key
        assert sa == sb, key
        assert fa[0] == 1 and fa[1] == 0 and fa == fb, key  # one prefilter launch, no overflow


@pytest.mark.gpu
def test_extreme_queries_find_their_planted_row_at_plus_zero(gpu_pkg, tmp_path_factory):
    for side in ("final", "recheck", "f32"):
        run = _side(tmp_path_factory, side)
        for key, B, nb, id_offset in ch.LAUNCHES:
            ids = run[key + "_i"].reshape(nb, B, ch.K + 1)
            bits = run[key + "_d"].view(np.uint32).reshape(nb, B, ch.K + 1)
            for qrow, row in ((ch.Q_LO, ch.ROW_LO), (ch.Q_HI, ch.ROW_HI)):
                assert (ids[:, qrow, 0] == row + id_offset).all(), (side, key, qrow)
                assert (bits[:, qrow, 0] == 0).all(), (side, key, qrow)  # +0.0
                assert (bits[:, qrow, 1] != 0).all(), (side, key, qrow)
