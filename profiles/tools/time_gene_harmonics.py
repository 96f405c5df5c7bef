#!/usr/bin/env python
"""Times the kernel behind Cycle.from_phases_mle (vc_gene_glm) with device events, after a warm-up, on a dense device block, and the
worker `velocycle_amd.gene_harmonics.gene_harmonics` end to end (staging, fit, null fit, lgamma constants) by the wall clock.

    python profiles/tools/time_gene_harmonics.py [--cells 50000] [--genes 2000] [--harmonics 1] [--reps 5] [--warmup 2] [--out FILE.json]

For Poisson / negative binomial and uint16 / float32 count storage it prints one JSON line: the median, minimum and maximum of `reps`
launches (each bracketed by its own pair of events), how the genes ended (status counts, Newton steps, passes over the cells = steps + 1
when no step was halved), and the bytes one pass reads per element (count + logm + 2H basis rows).  No GPU: it fails, it does not fall back."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from velocycle_amd import _lib                            # noqa: E402
from velocycle_amd.gene_harmonics import STATUS, fourier_basis_from_directions, gene_harmonics        # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--harmonics", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gene_harmonics.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, Ng, H = a.cells, a.genes, a.harmonics
    K, NH = 2 * H + 1, (2 * H + 1) * (H + 1)
    sim = simulate_counts(Nc=Nc, Ng=Ng, seed=21, device=dev)
    S = sim["S"]
    keep = S.sum(0) > 0
    S = S[:, keep].contiguous()
    Ng = int(S.shape[1])
    n = S.sum(1).clamp_min(1.0).double()
    phis = sim["phis"].double().cpu().numpy()
    xy = np.stack([np.cos(phis), np.sin(phis)])
    B_d = fourier_basis_from_directions(xy, H).float().to(dev).contiguous()
    logm_d = torch.log(n).float().contiguous()
    r_d = torch.full((Ng,), 1.0 / 0.3, dtype=torch.float32, device=dev)
    blk32 = S.T.contiguous()
    i = blk32.to(torch.int32)
    i[i >= 32768] -= 65536
    blk16 = i.to(torch.int16)
    del i
    out = dict(nu=torch.empty((Ng, K), dtype=torch.float64, device=dev), cov=torch.empty((Ng, NH), dtype=torch.float64, device=dev),
               ll=torch.empty(Ng, dtype=torch.float64, device=dev), dec=torch.empty(Ng, dtype=torch.float64, device=dev),
               it=torch.empty(Ng, dtype=torch.int32, device=dev), st=torch.empty(Ng, dtype=torch.int32, device=dev))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rows = []
    for noise in ("Poisson", "NegativeBinomial"):
        for kind, blk in ((_lib.VC_COUNTS_U16, blk16), (_lib.VC_COUNTS_F32, blk32)):
            def launch():
                rc = lib.vc_gene_glm(C.c_void_p(blk.data_ptr()), kind, Ng, Nc, Nc, C.c_void_p(B_d.data_ptr()), K, C.c_void_p(logm_d.data_ptr()),
                                     _lib.NOISE[noise], C.c_void_p(r_d.data_ptr()), None, None, 1e-10, 25,
                                     *[C.c_void_p(out[k].data_ptr()) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
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
            it, st = out["it"].cpu().numpy(), out["st"].cpu().numpy()
            elem = blk.element_size() + 4 + 4 * 2 * H
            row = {"noise": noise, "storage": "u16" if kind == _lib.VC_COUNTS_U16 else "f32", "cells": Nc, "genes": Ng, "harmonics": H,
                   "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps,
                   "warmup": a.warmup, "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)},
                   "steps_mean": float(it.mean()), "steps_max": int(it.max()), "bytes_per_element_and_pass": elem,
                   "bytes_read_if_no_step_was_halved": int((it + 1).sum()) * Nc * elem, "ms_per_pass": float(np.median(ms)) / (it.mean() + 1),
                   "board": board}
            print(json.dumps(row), flush=True)
            rows.append(row)
    # the worker end to end, once (host counts in, host results out)
    S_host = S.cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = gene_harmonics(S_host, xy, n.cpu().numpy(), harmonics=H, noisemodel="NegativeBinomial", dispersion=0.3)
    wall = time.perf_counter() - t0
    row = {"worker_wall_s": wall, "cells": Nc, "genes": Ng, "harmonics": H, "noise": "NegativeBinomial",
           "periodic_at_1e-3": int((fit.p_value < 1e-3).sum()), "board": board}
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
