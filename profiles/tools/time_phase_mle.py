#!/usr/bin/env python
"""Times the kernel behind Phases.from_cycle_mle (vc_phase_mle) with device events, after a warm-up, on a dense device block.

    python profiles/tools/time_phase_mle.py [--cells 50000] [--genes 2000] [--bins 100] [--reps 20] [--warmup 5] [--out FILE.json]

For Poisson / negative binomial and uint16 / float32 count storage it prints one JSON line: the median, minimum and maximum of
`reps` launches (each bracketed by its own pair of events), the logarithms the launch issues (bins * genes * cells for the negative
binomial plus one per (gene, cell) and bin tile; Poisson: one per (gene, cell) and bin tile), and the time the transcendental
unit alone would need at the rate profiles/r03_valu_rate.txt measured (3.5 ns per wave64 v_log_f32 and SIMD at >= 4 waves per SIMD,
1 024 SIMDs).  No GPU: it fails, it does not fall back."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from velocycle_amd import _lib                            # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402

NS_PER_WAVE_LOG = 3.5
SIMDS = 1024
BIN_TILE = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_phase_mle.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, Ng, bins = a.cells, a.genes, a.bins
    sim = simulate_counts(Nc=Nc, Ng=Ng, seed=21, device=dev)
    S = sim["S"]
    n = S.sum(1).clamp_min(1.0).double()
    nu = sim["nu"].double()
    phis = 2 * np.pi * torch.arange(bins, device=dev, dtype=torch.float64) / bins
    T = torch.stack([torch.ones_like(phis), torch.sin(phis), torch.cos(phis)], -1) @ nu.T
    T[:, :] -= torch.log(n.mean())
    s = T.mean()
    T_d = (T - s).float().contiguous()
    E_d = torch.exp(T - s).float().contiguous()
    m_d = (n * torch.exp(s)).float().contiguous()
    r_d = (1.0 / sim["shape_inv"].clamp_min(0.05)).float().contiguous()
    blk32 = S.T.contiguous()
    i = blk32.to(torch.int32)
    i[i >= 32768] -= 65536
    blk16 = i.to(torch.int16)
    del i, sim
    best = torch.empty(Nc, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    tiles = -(-bins // BIN_TILE)
    for noise in ("Poisson", "NegativeBinomial"):
        for kind, blk in ((_lib.VC_COUNTS_U16, blk16), (_lib.VC_COUNTS_F32, blk32)):
            def launch():
                rc = lib.vc_phase_mle(C.c_void_p(blk.data_ptr()), kind, Ng, Nc, Nc, C.c_void_p(T_d.data_ptr()), C.c_void_p(E_d.data_ptr()),
                                      bins, C.c_void_p(m_d.data_ptr()), _lib.NOISE[noise], C.c_void_p(r_d.data_ptr()),
                                      C.c_void_p(best.data_ptr()), None, stream)
                assert rc == 0, lib.vc_last_error(None)
            for _ in range(a.warmup):
                launch()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            logs = Ng * Nc * tiles + (bins * Ng * Nc if noise == "NegativeBinomial" else 0)
            floor_ms = logs / 64 * NS_PER_WAVE_LOG / SIMDS * 1e-6
            row = {"noise": noise, "storage": "u16" if kind == _lib.VC_COUNTS_U16 else "f32", "cells": Nc, "genes": Ng, "bins": bins,
                   "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps,
                   "warmup": a.warmup, "logs_issued": int(logs), "log_unit_floor_ms": floor_ms,
                   "time_over_log_floor": float(np.median(ms)) / floor_ms, "count_bytes_read": int(blk.numel() * blk.element_size() * tiles),
                   "board": board}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
