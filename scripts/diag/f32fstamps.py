"""Where a step of scan_f32f_kernel goes (diagnostic build: scripts/diag/build_stamps.sh, then run this from the tree's
root).  Every wave sums, over its steps, the shader-clock time between its steps' stamps (vs_scan.hip, VS_F32F_STAMP);
this prints, over the waves and steps of one SIFT-1M launch of 32 batches x 32 queries, the share of a step spent in the
vmcnt wait, in the barrier, in the unit's DMA issue and in the four tiles, and how far the waves of a workgroup are apart
in tile time.  The kernel stamps [sweeper][8 waves][16] under either organisation; with two 4-wave workgroups per CU (the
default at 32 batches; VSEARCH_F32F_WAVES=8 forces the other) waves 0..3 and 4..7 of a sweeper are workgroups of their own."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
pkg.LIB_PATH = os.path.abspath("scratch/stamps/libvsearch_hip.so")
L = pkg.lib()
L.vs_debug_buffer.argtypes = [C.c_void_p]
NB, B = 32, 32
base = pkg.synth_sift(1_000_000, seed=20251205)
q = pkg.synth_sift(NB * B, seed=20251206)
qd = torch.from_numpy(q).cuda()
st = torch.cuda.current_stream().cuda_stream
o_d = torch.zeros((NB * B, 6), dtype=torch.float32, device="cuda")
o_i = torch.zeros((NB * B, 6), dtype=torch.int32, device="cuda")
fl = torch.zeros((NB * B,), dtype=torch.int32, device="cuda")
ROW0 = 12288  # the kernel's rows of the debug buffer (the launches around it stamp the first rows)
dbg = torch.zeros((ROW0 + 256 * 8, 16), dtype=torch.int32, device="cuda")  # at most 256 sweepers of 8 waves (256 workgroups of 8, or 512 of 4)
L.vs_debug_buffer(dbg.data_ptr())
names = ["between steps", "vmcnt wait", "barrier", "DMA issue", "tile 0", "tile 1", "tile 2", "tile 3"]
with pkg.BruteForceIndex(base) as idx:
    idx.set_precision(1)
    for rep in range(3):
        dbg.zero_()
        idx.search_dev_multi(qd.data_ptr(), NB, B, 5, o_i.data_ptr(), o_d.data_ptr(), fl.data_ptr(), st)
        torch.cuda.synchronize()
    NW = 8 if os.environ.get("VSEARCH_F32F_WAVES") == "8" else 4  # waves per workgroup
    t = dbg.cpu().numpy().astype(np.int64)[ROW0:].reshape(256 * 8 // NW, NW, 16)
    t = t[t[:, 0, 8] != 0]  # workgroups that ran
    steps = t[:, :, 8]
    per_step = t[:, :, :8] / steps[:, :, None]  # clocks per step, by wave
    total = per_step.sum(2)
    print(f"workgroups {t.shape[0]} of {NW} waves, steps per wave {steps.mean():.1f}, clocks per step {total.mean():.0f} "
          f"(min wave {total.min():.0f}, max wave {total.max():.0f}), candidates per wave {t[:, :, 9].mean():.1f}")
    for i, n in enumerate(names):
        print(f"  {n:14s} {per_step[:, :, i].mean():9.1f} clocks  {100.0 * per_step[:, :, i].mean() / total.mean():5.1f} %")
    tiles = per_step[:, :, 4:].sum(2)  # [workgroup][wave]
    spread = (tiles.max(1) - tiles.min(1)) / tiles.mean(1)
    print(f"  tiles          {tiles.mean():9.1f} clocks  {100.0 * tiles.mean() / total.mean():5.1f} %")
    print(f"  tile time between the waves of a workgroup: (max - min) / mean = {100.0 * spread.mean():.1f} % on average, "
          f"{100.0 * spread.max():.1f} % at most; barrier + vmcnt wait = "
          f"{100.0 * (per_step[:, :, 1].mean() + per_step[:, :, 2].mean()) / total.mean():.1f} % of a step")
