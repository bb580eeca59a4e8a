"""The comparison of a search_dev_multi result (k + 1 best per query and a tie flag) with the oracle's k best, shared by
the tests that call the device-level API."""
import numpy as np


def check_dev_multi(gi, gd, f, oi, od, k=5):
    """gi, gd: [nq, k + 1] ids and distances, f: [nq] flags, oi, od: the oracle's [nq, k].  Unflagged queries: ids and
    distances bit for bit.  Flagged queries (equal distances among the k + 1 best): distances still exact, ids a valid
    tie order."""
    assert set(np.unique(f)) <= {0, 1}
    keep = f == 0
    assert keep.mean() > 0.9
    assert np.array_equal(gi[keep, :k], oi[keep]) and np.array_equal(gd[keep, :k], od[keep])
    assert np.array_equal(gd[:, :k], od)
    assert (np.diff(gd, axis=1) >= 0).all() and (gi >= 0).all()
