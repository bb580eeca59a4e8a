"""Where a step of scan_f32f_kernel goes (diagnostic build: scripts/diag/build_stamps.sh, then run this from the tree's
root).  Every wave sums, over its steps, the shader-clock time between its steps' stamps (vs_scan.hip, VS_F32F_STAMP);
this prints, over the waves and steps of one SIFT-1M launch of 32 batches x 32 queries, the share of a step spent in the
vmcnt wait, in the barrier, in the unit's DMA issue and in the four tiles, and how far the waves of a workgroup are apart
in tile time.  The kernel stamps [sweeper][8 waves][16] under either organisation; with two 4-wave workgroups per CU (the
default at 32 batches; VSEARCH_F32F_WAVES=8 forces the other) waves 0..3 and 4..7 of a sweeper are workgroups of their own.

    python3 scripts/diag/f32fstamps.py --ends [--lib PATH]

reads the light diagnostic build instead (scripts/diag/build_stamps.sh ends: -DVS_F32F_ENDS, three clock reads per wave
and none inside the loop, so the kernel runs at the product's speed): when every workgroup of that launch starts, leaves
its loop and ends, over the grid, per XCD and per half, and the share of the launch that a perfect balance could remove
-- (last end - mean end) / (last end - first start).  The two halves of the 4-wave organisation share a CU, so read the
share per half as well: what lies between the halves' ends is no imbalance between CUs.  VSEARCH_F32F_PRIO
sets the priority duty of half 1."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import __graft_entry__ as ge

pkg = ge.load_package()
ENDS = "--ends" in sys.argv
pkg.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv
                               else "scratch/ends/libvsearch_hip.so" if ENDS else "scratch/stamps/libvsearch_hip.so")
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
    if ENDS:
        raw = dbg.cpu().numpy()[ROW0:].reshape(256 * 8 // NW, NW, 16)  # [sweeper x, half z][wave]
        ran = np.flatnonzero((raw[:, 0, 0] != 0) | (raw[:, 0, 1] != 0))  # workgroups that ran: index = sweeper * (8 / NW) + half
        raw = raw[ran]
        clk = raw[:, :, :6].astype(np.int64) & 0xFFFFFFFF
        tick = (clk[:, :, 0::2] | (clk[:, :, 1::2] << 32)) * 0.01  # [workgroup][wave][start, loop end, end] in us (a 100 MHz clock)
        t0 = tick[:, :, 0].min()
        wg = np.stack([tick[:, :, 0].min(1), tick[:, :, 1].max(1), tick[:, :, 2].max(1)], 1) - t0  # a workgroup: first start, last wave out
        units, xcd = raw[:, 0, 6], raw[:, 0, 7]
        half = ran % (8 // NW)
        print(f"launch of {NB} batches, {raw.shape[0]} workgroups of {NW} waves, VSEARCH_F32F_PRIO={os.environ.get('VSEARCH_F32F_PRIO', 'unset')}; "
              f"us after the first start")

        def row(name, sel):
            w, u = wg[sel], units[sel]
            return (f"{name:10s} n {w.shape[0]:3d}  start {w[:, 0].mean():6.2f} [{w[:, 0].min():6.2f}, {w[:, 0].max():6.2f}]  "
                    f"loop end {w[:, 1].mean():7.2f} [{w[:, 1].min():7.2f}, {w[:, 1].max():7.2f}]  "
                    f"end {w[:, 2].mean():7.2f} [{w[:, 2].min():7.2f}, {w[:, 2].max():7.2f}]  "
                    f"units {u.mean():6.2f} [{u.min()}, {u.max()}]")

        print("mean [min, max]:")
        print(row("grid", np.ones(raw.shape[0], dtype=bool)))
        for x in sorted(set(xcd.tolist())):
            print(row(f"XCD {x}", xcd == x))
        for z in sorted(set(half.tolist())):
            print(row(f"half {z}", half == z))
        last, first = wg[:, 2].max(), wg[:, 0].min()
        print(f"launch {last - first:.2f} us; last end - mean end = {last - wg[:, 2].mean():.2f} us = "
              f"{100.0 * (last - wg[:, 2].mean()) / (last - first):.2f} % of the launch (what a perfect balance could remove); "
              f"last loop end - mean loop end = {wg[:, 1].max() - wg[:, 1].mean():.2f} us")
        print("per workgroup: sweeper half XCD units start loop_end end")
        for i in range(raw.shape[0]):
            print(f"{ran[i] // (8 // NW):4d} {half[i]} {xcd[i]} {units[i]:3d} {wg[i, 0]:7.2f} {wg[i, 1]:7.2f} {wg[i, 2]:7.2f}")
        sys.exit(0)
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
