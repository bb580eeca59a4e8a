"""Child process of test_gpu_stream_passes.py (the VSEARCH_* knobs are read when the library loads, so every knob setting
is a process of its own):  stream_passes_child.py <repository root> <data .npz> <precision> <cases>

cases = "nb:B,nb:B,..." on the large base, "s" + nb:B on the small one.  One search_dev_multi launch per case, compared
with the oracle's lists in the data file."""
import os
import sys

import numpy as np

root, data_path, precision, cases = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from dev_multi_check import check_dev_multi  # noqa: E402

K = 5
pkg = ge.load_package()
data = np.load(data_path)
dev = torch.device("cuda", 0)
qd = torch.from_numpy(data["q"]).to(dev)
stream = torch.cuda.current_stream().cuda_stream


def run(idx, nb, B, oi, od):
    nq = nb * B
    o_d = torch.zeros((nq, K + 1), dtype=torch.float32, device=dev)
    o_i = torch.full((nq, K + 1), -7, dtype=torch.int32, device=dev)
    fl = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    idx.search_dev_multi(qd.data_ptr(), nb, B, K, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), stream)
    torch.cuda.synchronize()
    try:
        check_dev_multi(o_i.cpu().numpy(), o_d.cpu().numpy(), fl.cpu().numpy(), oi[:nq], od[:nq], K)
    except AssertionError:
        print(f"FAILED: {nb} batches of {B}, precision {precision}", flush=True)
        raise


for small in (False, True):
    mine = [c.lstrip("s") for c in cases.split(",") if c.startswith("s") == small]
    if not mine:
        continue
    tag = "small_" if small else ""
    with pkg.BruteForceIndex(data[tag + "base"]) as idx:
        idx.set_precision(precision)
        for c in mine:
            nb, B = (int(x) for x in c.split(":"))
            run(idx, nb, B, data[tag + "oi"], data[tag + "od"])
print("STREAM_PASSES_OK")
