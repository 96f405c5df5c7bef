#!/usr/bin/env python
"""Times the kernel behind the per-cell and per-group angular speed (vc_cell_speed: one per-cell fit, one evaluate-only pass) next to
vc_gene_kinetics on the same dense device block, in one run on one board, with device events after a warm-up; then
`velocycle_amd.cell_speed.grouped_angular_speed` over phase bins end to end by the wall clock (host counts in, host result out: staging,
the lgamma constants, one evaluate-only pass per round, the group sums on the host).

    python profiles/tools/time_cell_speed.py [--cells 50000] [--genes 2000] [--bins 20] [--reps 3] [--warmup 1] [--out FILE.json]

The bench generator's unspliced counts at the coefficients of a vc_gene_glm fit of its spliced counts, H = 1, NegativeBinomial at
dispersion 0.3, uint16 counts; the kinetics and the start are `velocity_map`'s fit (one constant speed).  One JSON line per kernel:
median, minimum and maximum of `reps` launches (each bracketed by its own pair of events), how the cells ended, the steps and the time per
pass (start + steps; refused trials not counted).  No GPU: it fails, it does not fall back."""
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
from velocycle_amd.cell_speed import STATUS, grouped_angular_speed, phase_bin_groups      # noqa: E402
from velocycle_amd.gene_harmonics import fourier_basis_from_directions        # noqa: E402
from velocycle_amd.gene_kinetics import DEFAULT_PRIOR, velocity_map           # noqa: E402
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


def u16_bits(blk32):
    i = blk32.to(torch.int32)
    i[i >= 32768] -= 65536
    return i.to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_cell_speed.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, H, K, NH = a.cells, 1, 3, 6
    sim = simulate_counts(Nc=Nc, Ng=a.genes, seed=21, device=dev)
    keep = (sim["S"].sum(0) > 0) & (sim["U"].sum(0) > 0)
    S, U = sim["S"][:, keep].contiguous(), sim["U"][:, keep].contiguous()
    Ng = int(S.shape[1])
    n = S.sum(1).clamp_min(1.0).double()
    phis = sim["phis"].double().cpu().numpy()
    xy = np.stack([np.cos(phis), np.sin(phis)])
    B_d = fourier_basis_from_directions(xy, H).float().to(dev).contiguous()
    logm_d = torch.log(n).float().contiguous()
    r_d = torch.full((Ng,), 1.0 / 0.3, dtype=torch.float32, device=dev)
    W_d = torch.ones((1, Nc), dtype=torch.float32, device=dev)
    prior_d = torch.tensor(DEFAULT_PRIOR, dtype=torch.float64, device=dev).expand(Ng, 4).contiguous()
    sblk, ublk = u16_bits(S.T.contiguous()), u16_bits(U.T.contiguous())
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    glm = dict(nu=f64(Ng, K), cov=f64(Ng, NH), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng))
    kin = dict(xy=f64(Ng, 2), cov=f64(Ng, 3), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng), nc=i32(Ng), score=f64(Ng, 1), info=f64(Ng, 1))
    csp = dict(omega=f64(Nc), var=f64(Nc), sums=f64(Nc, 6), dec=f64(Nc), it=i32(Nc), st=i32(Nc), nc=i32(Nc))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    kind, noise = _lib.VC_COUNTS_U16, _lib.NOISE["NegativeBinomial"]
    rc = lib.vc_gene_glm(p(sblk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d), None, None, 1e-10, 25,
                         *[p(glm[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
    assert rc == 0, lib.vc_last_error(None)
    means = glm["nu"].T.cpu().numpy()
    U_host, n_host = U.cpu().numpy(), n.cpu().numpy()
    kw = dict(noisemodel="NegativeBinomial", dispersion=0.3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = velocity_map(U_host, xy, n_host, means, **kw)
    map_wall = time.perf_counter() - t0
    omega = float(fit.nu_omega[0, 0])
    good = np.isfinite(fit.kinetics.log_gamma) & np.isfinite(fit.kinetics.log_beta)
    xy_d = torch.as_tensor(np.stack([np.where(good, fit.kinetics.log_gamma, 0.0), np.where(good, fit.kinetics.log_beta, 2.0)], 1)).to(dev)
    nuw_d = torch.full((1,), omega, dtype=torch.float64, device=dev)
    start_d = torch.full((Nc,), omega, dtype=torch.float64, device=dev)

    def kinetics():
        rc = lib.vc_gene_kinetics(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(W_d), 1, p(nuw_d), noise, p(r_d),
                                  p(prior_d), None, 1e-10, 25,
                                  *[p(kin[k]) for k in ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")], stream)
        assert rc == 0, lib.vc_last_error(None)

    def cells(max_iter):
        rc = lib.vc_cell_speed(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(xy_d), noise, p(r_d), None, p(start_d),
                               1e-10, max_iter, *[p(csp[k]) for k in ("omega", "var", "sums", "dec", "it", "st", "nc")], stream)
        assert rc == 0, lib.vc_last_error(None)

    rows = []
    base = {"noise": "NegativeBinomial", "storage": "u16", "cells": Nc, "genes": Ng, "harmonics": H, "omega": omega, "board": board}
    t = timed(kinetics, a.warmup, a.reps)
    rows.append({"kernel": "vc_gene_kinetics", **base, **t, "steps_mean": float(kin["it"].double().mean())})
    for label, max_iter in (("vc_cell_speed, per-cell fit", 25), ("vc_cell_speed, evaluate-only", 0)):
        t = timed(lambda: cells(max_iter), a.warmup, a.reps)
        it, st = csp["it"].cpu().numpy(), csp["st"].cpu().numpy()
        om = csp["omega"].cpu().numpy()
        passes = 1.0 + float(it.max())                     # a workgroup runs until its last cell has stopped
        rows.append({"kernel": label, **base, **t, "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)},
                     "steps_mean": float(it.mean()), "steps_max": int(it.max()), "passes_at_least": passes,
                     "ms_per_pass_at_most": t["ms_median"] / passes, "omega_median": float(np.nanmedian(om)),
                     "omega_iqr": [float(np.nanpercentile(om, 25)), float(np.nanpercentile(om, 75))],
                     "clamped_genes_per_cell": float(csp["nc"].double().mean())})
    groups, centres = phase_bin_groups(xy, a.bins)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    g = grouped_angular_speed(U_host, xy, n_host, means, fit.kinetics.log_gamma, fit.kinetics.log_beta, groups, omega, **kw)
    t2 = time.perf_counter()
    rows.append({"worker": "grouped_angular_speed", **base, "bins": a.bins, "worker_wall_s": t2 - t1, "velocity_map_wall_s": map_wall,
                 "genes_kept": int(good.sum()), "omega": g.omega.tolist(), "stds": g.stds.tolist(), "rounds": g.rounds.tolist(),
                 "status": [STATUS[int(s)] for s in g.status], "n_cells": g.n_cells.tolist(), "n_clamped": g.n_clamped.tolist(),
                 "velocity_map_omega": omega, "velocity_map_std": float(fit.stds[0, 0])})
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
