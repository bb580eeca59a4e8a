"""The bf16 row image of the prefilter (row_filter_image_kernel, scan_f32f_kernel on 64-row units) against
scan_f32s_kernel (VSEARCH_F32_FILTER=0), bit for bit, at the smallest shard that takes the prefilter (4096 tiles: a
workgroup has 4 or 5 units): row counts that end 0, 1, 15, 17, 31 and 63 rows past a unit, winners planted in the first
and the last unit, queries far smaller than every row (the image's zero spare rows would win if a tail were not masked),
and rows whose bf16 rounding is a tie on every element.  Each side runs once, in a process of its own; the tests share
the two result files."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (also run as a script: the A/B worker below)
    sys.path.insert(0, ROOT)

# rows of the ragged cases: tails of 0, 1, 15, 17, 31, 63 rows past a 64-row unit, and one unit more with a one-row tail
RAGGED_ROWS = (65_536, 65_537, 65_551, 65_553, 65_567, 65_599, 69_633)
# (metric, queries per batch, batch counts) for every row count
RAGGED_RUNS = ((0, 32, (1, 5, 8, 17, 32)), (1, 32, (1, 5, 8, 17, 32)), (0, 20, (8,)))
EDGE_ROWS = 65_599        # 63 rows in the last unit
PAD_ROWS, PAD_OFFSET = 65_537, 1_000_000
TIE_ROWS = 65_553


def _ragged_data(rows, seed):
    """Gaussian rows, queries near rows, 12 near-duplicates 2^-20 apart per query around its 5th / 6th best (the ring test's)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((rows, 128)).astype(np.float32)
    q = (g[rng.integers(0, rows, 32 * 32)] + 0.3 * rng.standard_normal((32 * 32, 128))).astype(np.float32)
    u = rng.standard_normal((256, 128))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    for m in range(12):
        g[256 * m: 256 * (m + 1)] = (q[:256] + (1.0 + m * 2.0 ** -20) * u).astype(np.float32)
    return g, q


def _edge_data(metric):
    """One batch whose 6 best rows per query sit in the first 16 rows and in the last rows % 64 rows: query j's
    neighbours are rows e[0..5] at strictly increasing distance (L2) / decreasing product (IP)."""
    rng = np.random.default_rng(7 + metric)
    rows = EDGE_ROWS
    g = rng.standard_normal((rows, 128)).astype(np.float32)
    tail = rows % 64
    c = rng.standard_normal(128)
    c /= np.linalg.norm(c)
    # the planted rows lie along c at six distinct lengths; the queries along c as well, so that their order is the lengths'
    pick = np.concatenate([rng.choice(16, 3, replace=False), rows - tail + rng.choice(tail, 3, replace=False)])
    rng.shuffle(pick)
    want = np.empty((32, 6), np.int64)
    q = np.empty((32, 128), np.float32)
    if metric == 0:
        for m, row in enumerate(pick):
            g[row] = (40.0 + 0.25 * m) * c      # far from the gaussian cloud (norm ~ 11.3), 0.25 apart
        for j in range(32):
            q[j] = (39.0 - 0.01 * j) * c        # nearest: length 40, then 40.25, ...
            want[j] = pick
    else:
        for m, row in enumerate(pick):
            g[row] = (60.0 - 2.0 * m) * c       # products (60 - 2 m) |q| against ~ N(0, |q|^2) elsewhere
        for j in range(32):
            q[j] = (1.0 + 0.01 * j) * c
            want[j] = pick
    return g, q, want


def _pad_data():
    rng = np.random.default_rng(11)
    g = rng.standard_normal((PAD_ROWS, 128)).astype(np.float32)
    q = (1e-3 * rng.standard_normal((32, 128))).astype(np.float32)  # |q|^2 ~ 1e-4: a zero row would be nearest by far
    return g, q


def _tie_data():
    """Every value's low 16 mantissa bits are 0x8000 and the bit above alternates, so that round-to-nearest-even goes
    up on every other element and down on the rest: truncation, round-half-up and RNE all give different images."""
    rng = np.random.default_rng(13)
    g = rng.standard_normal((TIE_ROWS, 128)).astype(np.float32)
    bits = g.view(np.uint32)
    odd = (np.arange(TIE_ROWS * 128, dtype=np.uint32).reshape(TIE_ROWS, 128) & 1) << 16
    bits[:] = (bits & np.uint32(0xFFFE0000)) | odd | np.uint32(0x8000)
    q = (g[rng.integers(0, TIE_ROWS, 5 * 32)] + 0.3 * rng.standard_normal((5 * 32, 128))).astype(np.float32)
    return g, q


def _search(idx, torch, dev, q, nb, B):
    qd = torch.from_numpy(np.ascontiguousarray(q[: nb * B])).to(dev)
    o_d = torch.zeros((nb * B, 6), dtype=torch.float32, device=dev)
    o_i = torch.full((nb * B, 6), -7, dtype=torch.int32, device=dev)
    fl = torch.full((nb * B,), -7, dtype=torch.int32, device=dev)
    idx.search_dev_multi(qd.data_ptr(), nb, B, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy()


def _worker(argv):
    """python test_f32_filter_image.py <out.npz>: the searches of one A/B side, in a process of its own."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    res = {}

    def put(key, out):
        res[key + "_i"], res[key + "_d"], res[key + "_f"] = out

    for ri, rows in enumerate(RAGGED_ROWS):
        base, q = _ragged_data(rows, 300 + ri)
        for metric, B, nbs in RAGGED_RUNS:
            with pkg.BruteForceIndex(base, metric=metric) as idx:
                idx.set_precision(1)
                for nb in nbs:
                    put(f"ragged_{rows}_m{metric}_B{B}_nb{nb}", _search(idx, torch, dev, q, nb, B))
    for metric in (0, 1):
        base, q, _ = _edge_data(metric)
        with pkg.BruteForceIndex(base, metric=metric) as idx:
            idx.set_precision(1)
            put(f"edge_m{metric}", _search(idx, torch, dev, q, 1, 32))
    base, q = _pad_data()
    with pkg.BruteForceIndex(base, id_offset=PAD_OFFSET) as idx:
        idx.set_precision(1)
        put("pad", _search(idx, torch, dev, q, 1, 32))
    base, q = _tie_data()
    with pkg.BruteForceIndex(base) as idx:
        idx.set_precision(1)
        put("tie", _search(idx, torch, dev, q, 5, 32))
    np.savez(argv[0], **res)


@pytest.fixture(scope="module")
def sides(gpu_pkg, tmp_path_factory):
    """(prefilter on its image, scan_f32s_kernel): every search of this file, once per side."""
    out = []
    for flt in (1, 0):
        path = str(tmp_path_factory.mktemp("image") / f"side_{flt}.npz")
        # every batch count takes the seeded streaming scan (the default seeds from 4 batches on)
        env = dict(os.environ, VSEARCH_F32_FILTER=str(flt), VSEARCH_SEED_MIN="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=900)
        out.append(dict(np.load(path)))
    assert out[0].keys() == out[1].keys()
    return out


def _equal(sides, prefix):
    a, b = sides
    keys = [k for k in a if k.startswith(prefix)]
    assert keys
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("rows", RAGGED_ROWS)
def test_ragged_units_equal_fp32_kernel_bit_for_bit(sides, rows):
    keys = _equal(sides, f"ragged_{rows}_")
    assert len(keys) == 3 * sum(len(nbs) for _, _, nbs in RAGGED_RUNS)
    ids = sides[0][f"ragged_{rows}_m0_B32_nb32_i"][:, :5]
    assert ((ids >= 0) & (ids < rows)).all()  # the lists are not empty


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [0, 1])
def test_winners_in_the_first_and_last_unit(sides, metric):
    _equal(sides, f"edge_m{metric}")
    _, _, want = _edge_data(metric)
    got = sides[0][f"edge_m{metric}_i"]
    assert np.array_equal(got, want), "the planted rows, in order"
    tail = EDGE_ROWS % 64
    assert (want < 16).any() and (want >= EDGE_ROWS - tail).any()
    assert (sides[0][f"edge_m{metric}_f"] == 0).all()


@pytest.mark.gpu
def test_spare_rows_of_the_image_never_surface(sides):
    _equal(sides, "pad")
    ids = sides[0]["pad_i"]
    assert ((ids >= PAD_OFFSET) & (ids < PAD_OFFSET + PAD_ROWS)).all()
    assert np.isfinite(sides[0]["pad_d"]).all() and (sides[0]["pad_d"] > 10.0).all()  # |b|^2 ~ 128, never a zero row's |q|^2


@pytest.mark.gpu
def test_image_rounds_ties_to_even_like_the_statistics(sides):
    """Bit-equal on rows whose rounding is a tie everywhere.  The library exports no count of dropped or overflowed
    entries and the overflow fallback gives the same outputs, so this is an A/B on tie data only: no query skipped
    (flags <= 1) and the outputs those of the fp32 kernel.  That the image is rounded to nearest even, as the statistics
    assume, is pinned by test_image_is_numpy_rne_in_fragment_order on the image itself."""
    _equal(sides, "tie")
    assert sides[0]["tie_f"].max() <= 1 and sides[0]["tie_f"].min() >= 0
    ids = sides[0]["tie_i"][:, :5]
    assert ((ids >= 0) & (ids < TIE_ROWS)).all()


def _image_reference(x):
    """Rows of floats -> the image: bf16 by round to nearest even, 16-byte chunk 4 s + g of a row = k 32 s + 4 g + i
    (elements 0..3) and 32 s + 16 + 4 g + i (4..7)."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    bf = ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    # [row][s][u][g][i] -> [row][s][g][u][i]
    return bf.reshape(-1, 4, 2, 4, 4).transpose(0, 1, 3, 2, 4).reshape(-1, 128)


@pytest.mark.gpu
def test_image_is_numpy_rne_in_fragment_order(gpu_pkg):
    """The image itself, read back: every element is the row's value rounded to nearest even (ties included: the tie
    rows differ from truncation and from round-half-up on every other element), every 16-byte chunk holds the k values
    its lane feeds the MFMA, and the 64 spare rows are zero."""
    base, _ = _tie_data()
    rng = np.random.default_rng(17)
    base[1::2] = rng.standard_normal((len(base[1::2]), 128)).astype(np.float32)  # every other row ordinary values
    base[3, :] = np.arange(128, dtype=np.float32)                               # a row that names its own k
    with gpu_pkg.BruteForceIndex(base) as idx:
        img = idx.filter_image(0, TIE_ROWS + 64)
    assert np.array_equal(img[:TIE_ROWS], _image_reference(base))
    assert not img[TIE_ROWS:].any()
    k = img[3].astype(np.uint32) << 16
    assert np.array_equal(k.view(np.float32)[:8], np.array([0, 1, 2, 3, 16, 17, 18, 19], np.float32))


if __name__ == "__main__":
    _worker(sys.argv[1:])
