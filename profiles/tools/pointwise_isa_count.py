#!/usr/bin/env python
"""Static instruction counts of the draw loop of vc_pointwise_kernel from the emitted gfx950 assembly.

    python profiles/tools/pointwise_isa_count.py [FILE.s]

Without FILE.s it compiles velocycle_amd/csrc/vc_pointwise.hip with `hipcc -S --cuda-device-only` (the Makefile's flags) first.  Per
instantiation it prints the code object's register and scratch metadata, and for the draw loop -- the SHORTEST backward-branch region
of the kernel that holds at least 2 transcendentals per tile cell -- the vector instructions, the transcendentals among them
(v_exp / v_log / v_rcp / v_rsq / v_sqrt), lane moves (v_readlane / v_writelane), vector memory loads, and both per element-draw
(divided by the tile's cells TC).  The region is one path through the loop body: a branch inside it (record recomputed or not) is
counted as laid out, so the figures are an estimate, good to a few instructions per element-draw."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KIND = {0: "phase", 1: "velocity", 2: "velocity, S once"}
NOISE = {0: "NB", 1: "Poisson"}


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        path = os.path.join(tempfile.mkdtemp(), "pw.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "velocycle_amd", "csrc", "vc_pointwise.hip"), "-o", path], check=True, capture_output=True)
    txt = open(path).read()
    L = txt.split("\n")
    meta = {m.group(1): m.groups()[1:] for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n"
        r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt)}
    print("H kind noise storage TC | scratch vgpr sgpr_parked_in_vgpr_lanes | loop: v_ trans lane_moves vmem | per element-draw: valu trans")
    for i, l in enumerate(L):
        m = re.match(r"^(_ZN\S*vc_pointwise_kernelILi(\d)ELi(\d)ELi(\d)ELb(\d)ELi(\d)E\S*):", l)
        if not m:
            continue
        name, H, kind, noise, u16, tc = m.group(1), *map(int, m.groups()[1:])
        end = next(j for j in range(i, len(L)) if "s_endpgm" in L[j])
        body = L[i:end]
        labels = {mm.group(1): j for j, x in enumerate(body) for mm in [re.match(r"^(\.LBB\d+_\d+):", x)] if mm}
        cands = []
        for j, x in enumerate(body):
            mm = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", x)
            if mm and labels.get(mm.group(1), j) < j:
                seg = body[labels[mm.group(1)]:j]
                nt = sum(1 for y in seg if re.match(r"\s+v_(exp|log|rcp|rsq|sqrt)_", y))
                if nt >= 2 * tc:
                    cands.append((len(seg), nt, seg))
        n, nt, seg = min(cands, key=lambda c: c[0])
        nv = sum(1 for y in seg if re.match(r"\s+v_", y))
        lm = sum(1 for y in seg if "readlane" in y or "writelane" in y)
        vm = sum(1 for y in seg if re.match(r"\s+(global|flat)_load", y))
        sc, sg, ss, vg, vs = meta.get(name, ("?",) * 5)
        print(f"{H} {KIND[kind]:17s} {NOISE[noise]:7s} {'u16' if u16 else 'f32'} {tc} | {sc} {vg} {ss} | {nv} {nt} {lm} {vm} | "
              f"{(nv - nt) / tc:.1f} {nt / tc:.2f}")


if __name__ == "__main__":
    main()
