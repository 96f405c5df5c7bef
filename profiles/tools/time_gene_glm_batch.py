#!/usr/bin/env python
"""Times the kernel behind Cycle.from_phases_batch_mle (vc_gene_glm_batch) next to vc_gene_glm, in one run on one board, with device
events after a warm-up, on the same dense device block; and the worker `velocycle_amd.gene_batch.gene_harmonics_batched` end to end
(sorting, staging, fit, null fit, lgamma constants) by the wall clock.

    python profiles/tools/time_gene_glm_batch.py [--cells 50000] [--genes 2000] [--harmonics 1] [--batches 4] [--reps 5] [--warmup 2] [--out FILE.json]

Negative binomial, uint16 counts.  The batches are equal contiguous runs of cells; the simulated counts carry no batch effect, so the
fitted offsets are near 0 and both kernels do the same number of Newton steps' worth of passes.  One JSON line per kernel: median,
minimum and maximum of `reps` launches (each bracketed by its own pair of events), how the genes ended, the steps, and the time per
pass = median / (mean steps + 1).  No GPU: it fails, it does not fall back."""
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
from velocycle_amd.gene_batch import gene_harmonics_batched                                           # noqa: E402
from velocycle_amd.gene_harmonics import STATUS, fourier_basis_from_directions                        # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--harmonics", type=int, default=1)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gene_glm_batch.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, H, Nb = a.cells, a.harmonics, a.batches
    K, NH = 2 * H + 1, (2 * H + 1) * (H + 1)
    sim = simulate_counts(Nc=Nc, Ng=a.genes, seed=21, device=dev)
    S = sim["S"]
    S = S[:, S.sum(0) > 0].contiguous()
    Ng = int(S.shape[1])
    n = S.sum(1).clamp_min(1.0).double()
    phis = sim["phis"].double().cpu().numpy()
    xy = np.stack([np.cos(phis), np.sin(phis)])
    B_d = fourier_basis_from_directions(xy, H).float().to(dev).contiguous()
    logm_d = torch.log(n).float().contiguous()
    r_d = torch.full((Ng,), 1.0 / 0.3, dtype=torch.float32, device=dev)
    i = S.T.contiguous().to(torch.int32)
    i[i >= 32768] -= 65536
    blk = i.to(torch.int16)
    del i
    bounds = [Nc * b // Nb for b in range(Nb + 1)]
    seg = (C.c_int64 * (Nb + 1))(*bounds)
    dm = torch.zeros((Ng, Nb), dtype=torch.float64, device=dev)
    dq = torch.full((Ng, Nb), 4.0, dtype=torch.float64, device=dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)                                   # noqa: E731
    out = dict(nu=f64(Ng, K), delta=f64(Ng, Nb), cov=f64(Ng, NH), dvar=f64(Ng, Nb), ll=f64(Ng), dec=f64(Ng),
               it=torch.empty(Ng, dtype=torch.int32, device=dev), st=torch.empty(Ng, dtype=torch.int32, device=dev))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                                             # noqa: E731
    noise = _lib.NOISE["NegativeBinomial"]

    def plain():
        rc = lib.vc_gene_glm(p(blk), _lib.VC_COUNTS_U16, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d), None, None, 1e-10, 25,
                             *[p(out[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
        assert rc == 0, lib.vc_last_error(None)

    def batched():
        rc = lib.vc_gene_glm_batch(p(blk), _lib.VC_COUNTS_U16, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d), Nb, seg, p(dm), p(dq), None,
                                   None, 1e-10, 25, *[p(out[k]) for k in ("nu", "delta", "cov", "dvar", "ll", "dec", "it", "st")], stream)
        assert rc == 0, lib.vc_last_error(None)

    rows = []
    for name, launch in (("vc_gene_glm", plain), ("vc_gene_glm_batch", batched)):
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
        row = {"kernel": name, "noise": "NegativeBinomial", "storage": "u16", "cells": Nc, "genes": Ng, "harmonics": H,
               "batches": Nb if name.endswith("batch") else 0, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
               "ms_max": float(np.max(ms)), "reps": a.reps, "warmup": a.warmup,
               "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)}, "steps_mean": float(it.mean()),
               "steps_max": int(it.max()), "ms_per_pass": float(np.median(ms)) / (it.mean() + 1), "board": board}
        if name.endswith("batch"):
            row["max_abs_delta"] = float(out["delta"].abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the worker end to end, once (host counts in, host results out)
    S_host = S.cpu().numpy()
    labels = np.repeat(np.arange(Nb), np.diff(bounds))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = gene_harmonics_batched(S_host, xy, n.cpu().numpy(), labels, harmonics=H, noisemodel="NegativeBinomial", dispersion=0.3)
    wall = time.perf_counter() - t0
    row = {"worker_wall_s": wall, "cells": Nc, "genes": Ng, "harmonics": H, "batches": Nb, "noise": "NegativeBinomial",
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
