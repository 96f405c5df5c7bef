#!/usr/bin/env python
"""Times the kernel behind `gene_dispersion` / `gene_harmonics(dispersion="mle")` (vc_gene_dispersion) with device events, after a
warm-up, on a dense device block at the coefficients of a vc_gene_glm fit at dispersion 0.3, and the workers end to end by the wall
clock: `gene_harmonics` at the fixed dispersion 0.3 (what profiles/r14_gene_harmonics.md timed) and with dispersion="mle".

    python profiles/tools/time_gene_dispersion.py [--cells 50000] [--genes 2000] [--harmonics 1] [--reps 5] [--warmup 2] [--out FILE.json]

Prints one JSON line per timing: for uint16 / float32 storage the median, minimum and maximum of `reps` launches of each kernel (each
bracketed by its own pair of events), how the genes ended and the passes over the cells (2 bound checks + steps + 1; the first walk
that builds the histogram not counted); then the two workers.  No GPU: it fails, it does not fall back."""
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
from velocycle_amd.gene_harmonics import DISPERSION_STATUS, fourier_basis_from_directions, gene_harmonics        # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402


def timed(launch, warmup, reps):
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": reps, "warmup": warmup}


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
        raise SystemExit("time_gene_dispersion.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, Ng, H = a.cells, a.genes, a.harmonics
    K, NH = 2 * H + 1, (2 * H + 1) * (H + 1)
    sim = simulate_counts(Nc=Nc, Ng=Ng, seed=21, device=dev)
    S = sim["S"]
    S = S[:, S.sum(0) > 0].contiguous()
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
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda: torch.empty(Ng, dtype=torch.int32, device=dev)                      # noqa: E731
    glm = dict(nu=f64(Ng, K), cov=f64(Ng, NH), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32())
    dsp = dict(rho=f64(Ng), r=torch.empty(Ng, dtype=torch.float32, device=dev), info=f64(Ng), ll=f64(Ng), score=f64(Ng), it=i32(), st=i32())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    rows = []
    for kind, blk in ((_lib.VC_COUNTS_U16, blk16), (_lib.VC_COUNTS_F32, blk32)):
        def launch_glm():
            rc = lib.vc_gene_glm(p(blk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), _lib.NOISE["NegativeBinomial"], p(r_d), None, None, 1e-10, 25,
                                 *[p(glm[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
            assert rc == 0, lib.vc_last_error(None)

        def launch_dsp():
            rc = lib.vc_gene_dispersion(p(blk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(r_d), None, None, 1e-10, 50,
                                        *[p(dsp[k]) for k in ("rho", "r", "info", "ll", "score", "it", "st")], stream)
            assert rc == 0, lib.vc_last_error(None)
        storage = "u16" if kind == _lib.VC_COUNTS_U16 else "f32"
        row = {"kernel": "vc_gene_glm", "noise": "NegativeBinomial", "storage": storage, "cells": Nc, "genes": Ng, "harmonics": H,
               **timed(launch_glm, a.warmup, a.reps), "steps_mean": float(glm["it"].float().mean()), "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
        t = timed(launch_dsp, a.warmup, a.reps)
        it, st = dsp["it"].cpu().numpy(), dsp["st"].cpu().numpy()
        bound = (st == _lib.VC_DISP_AT_UPPER) | (st == _lib.VC_DISP_AT_LOWER)
        passes = np.where(st == _lib.VC_DISP_AT_UPPER, 1, np.where(bound, 2, it + 3))
        row = {"kernel": "vc_gene_dispersion", "storage": storage, "cells": Nc, "genes": Ng, "harmonics": H, **t,
               "status": {DISPERSION_STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)}, "steps_mean": float(it.mean()),
               "steps_max": int(it.max()), "passes_mean": float(passes.mean()), "ms_per_pass": t["ms_median"] / float(passes.mean()),
               "dispersion_quantiles_5_50_95": [float(q) for q in np.quantile(1.0 / dsp["r"].double().cpu().numpy(), [0.05, 0.5, 0.95])],
               "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the workers end to end, once each (host counts in, host results out)
    S_host, n_host = S.cpu().numpy(), n.cpu().numpy()
    for disp in (0.3, "mle"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = gene_harmonics(S_host, xy, n_host, harmonics=H, noisemodel="NegativeBinomial", dispersion=disp)
        wall = time.perf_counter() - t0
        row = {"worker_wall_s": wall, "dispersion": disp, "cells": Nc, "genes": Ng, "harmonics": H, "noise": "NegativeBinomial",
               "periodic_at_1e-3": int((fit.p_value < 1e-3).sum()), "board": board}
        if disp == "mle":
            row.update(rounds_max=int(fit.rounds.max()), rounds_mean=float(fit.rounds.mean()),
                       status={DISPERSION_STATUS[int(s)]: int((fit.dispersion_status == s).sum()) for s in np.unique(fit.dispersion_status)},
                       **{"overdispersed_at_1e-3": int((fit.overdispersion_p < 1e-3).sum())})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
