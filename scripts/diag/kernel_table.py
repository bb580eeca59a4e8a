#!/usr/bin/env python3
"""Per-kernel resources and instruction mix of two device-assembly builds, side by side.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S vs_scan.hip -o child/vs_scan.s   (same for the parent)
    kernel_table.py parent/vs_scan.s child/vs_scan.s [more pairs ...]

One row per kernel: VGPRs, AGPRs, SGPRs, scratch bytes, static LDS bytes, occupancy (the compiler's "Kernel info"
block), then the counts of v_mfma*, global_load_lds*, global_load_dword* (register loads), ds_read*/ds_load* and of all
v_* instructions, and the number of instructions that name M0 outside an inline-asm block.  A row whose parent and
child columns differ is marked with '*'; scalar instructions and s_nop are not compared.  Exit status 1 if any row is
marked.
"""
import collections
import re
import subprocess
import sys

INFO = [("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"),
        ("lds", "LDSByteSize"), ("occ", "Occupancy")]
MIX = [("mfma", r"v_mfma"), ("lds_dma", r"global_load_lds"), ("gload", r"global_load_dword"), ("ds_rd", r"ds_(read|load)"),
       ("valu", r"v_")]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def load(path):
    kernels = collections.OrderedDict()
    name, in_asm, in_info = None, False, False
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            kernels[name] = collections.Counter()
            in_asm = in_info = False
            continue
        if name is None:
            continue
        row = kernels[name]
        if line.startswith("; Kernel info:"):
            in_info = True
        elif in_info:
            m = re.match(r"^; (\w+)\s*:\s*(\d+)", line)
            if m:
                for key, tag in INFO:
                    if m.group(1) == tag:
                        row[key] = int(m.group(2))
            elif not line.startswith(";"):
                name = None
        elif "#ASMSTART" in line:
            in_asm = True
        elif "#ASMEND" in line:
            in_asm = False
        elif line.startswith("\t") and not line.startswith(("\t.", "\t;")):
            ins = line.split(";")[0].strip()
            op = ins.split()[0]
            for key, pat in MIX:
                if re.match(pat, op):
                    row[key] += 1
            if not in_asm and re.search(r"\bm0\b", ins):
                row["m0_out"] += 1
    return collections.OrderedDict((k, v) for k, v in kernels.items() if "vgpr" in v)


def main(argv):
    if len(argv) < 3 or len(argv) % 2 == 0:
        sys.exit(__doc__)
    cols = [k for k, _ in INFO] + [k for k, _ in MIX]
    marked = 0
    print("columns: parent/child of " + " ".join(cols) + " | m0 named outside inline asm (child)")
    for pa, ch in zip(argv[1::2], argv[2::2]):
        a, b = load(pa), load(ch)
        names = demangle(list(a))
        print("== %s | %s: %d kernels" % (pa, ch, len(a)))
        if list(a) != list(b):
            print("* the two files do not hold the same kernels")
            marked += 1
        for k in a:
            if k not in b:
                continue
            diff = any(a[k][c] != b[k][c] for c in cols)
            marked += diff
            short = re.sub(r"^void vs::|\(.*$", "", names[k])
            print("%s %-52s %s | %d" % ("*" if diff else " ", short, " ".join("%d/%d" % (a[k][c], b[k][c]) for c in cols), b[k]["m0_out"]))
    print("%d rows differ" % marked)
    return 1 if marked else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
