#!/usr/bin/env python
"""Times the kernel behind the cell bootstrap of the joint fit (vc_gene_joint_weighted, R rows of Poisson(1) case weights, every row from
the two-stage start) next to vc_gene_joint from the same start on the same dense device blocks, in one run on one board, with device
events after a warm-up; then `velocycle_amd.joint_bootstrap.velocity_map_joint_bootstrap` end to end by the wall clock (host counts in,
host result out) at tol_outer 1e-8 and 1e-6, with how the replicates ended.

    python profiles/tools/time_gene_joint_bootstrap.py [--cells 50000] [--genes 2000] [--rows 200] [--reps 3] [--warmup 1] [--out FILE.json]

The bench generator's counts, H = 1, NegativeBinomial at dispersion 0.3, uint16 counts; omega is `velocity_map`'s fit at the coefficients
of a vc_gene_glm fit of the spliced counts (the two-stage route), which is also the start of both kernels.  One JSON line per kernel and
per bootstrap.  No GPU: it fails, it does not fall back."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from velocycle_amd import _lib                            # noqa: E402
from velocycle_amd.gene_bootstrap import draw_weights     # noqa: E402
from velocycle_amd.gene_harmonics import fourier_basis_from_directions        # noqa: E402
from velocycle_amd.gene_joint import STATUS, velocity_map_joint               # noqa: E402
from velocycle_amd.gene_kinetics import DEFAULT_PRIOR, velocity_map           # noqa: E402
from velocycle_amd.joint_bootstrap import velocity_map_joint_bootstrap        # noqa: E402
from velocycle_amd.phase_mle import u16_bits              # noqa: E402
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
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gene_joint_bootstrap.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, H, K, NH, D, R = a.cells, 1, 3, 6, 5, a.rows
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
    pm_d = torch.zeros((Ng, K), dtype=torch.float64, device=dev)
    pp_d = torch.full((Ng, K), 1.0 / 9.0, dtype=torch.float64, device=dev)
    sblk, ublk = u16_bits(S.T.contiguous()), u16_bits(U.T.contiguous())
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    glm = dict(nu=f64(Ng, K), cov=f64(Ng, NH), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng))
    kin = dict(xy=f64(Ng, 2), cov=f64(Ng, 3), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng), nc=i32(Ng), score=f64(Ng, 1), info=f64(Ng, 1))
    names = ("theta", "cov", "lls", "llu", "dec", "it", "st", "nc", "score", "info")
    one = dict(theta=f64(Ng, D), cov=f64(Ng, D * (D + 1) // 2), lls=f64(Ng), llu=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng), nc=i32(Ng),
               score=f64(Ng, 1), info=f64(Ng, 1))
    many = dict(theta=f64(R, Ng, D), cov=None, lls=f64(R, Ng), llu=f64(R, Ng), dec=f64(R, Ng), it=i32(R, Ng), st=i32(R, Ng), nc=i32(R, Ng),
                score=f64(R, Ng, 1), info=f64(R, Ng, 1))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                 # noqa: E731
    kind, noise = _lib.VC_COUNTS_U16, _lib.NOISE["NegativeBinomial"]
    rc = lib.vc_gene_glm(p(sblk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d), None, None, 1e-10, 25,
                         *[p(glm[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
    assert rc == 0, lib.vc_last_error(None)
    means = glm["nu"].T.cpu().numpy()
    S_host, U_host, n_host = S.cpu().numpy(), U.cpu().numpy(), n.cpu().numpy()
    kw = dict(noisemodel="NegativeBinomial", dispersion=0.3)
    omega = float(velocity_map(U_host, xy, n_host, means, **kw).nu_omega[0, 0])
    nuw_d = torch.full((1,), omega, dtype=torch.float64, device=dev)
    rc = lib.vc_gene_kinetics(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(W_d), 1, p(nuw_d), noise, p(r_d), p(prior_d),
                              None, 1e-10, 25, *[p(kin[k]) for k in ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")], stream)
    assert rc == 0, lib.vc_last_error(None)
    start = torch.cat([glm["nu"], kin["xy"]], 1).contiguous()
    Wt = draw_weights(R, Nc, 0, dev)

    def plain():
        rc = lib.vc_gene_joint(p(sblk), p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(W_d), 1, p(nuw_d), noise, p(r_d), p(pm_d), p(pp_d),
                               p(prior_d), p(start), 1e-10, 40, *[p(one[k]) for k in names], stream)
        assert rc == 0, lib.vc_last_error(None)

    def weighted():
        rc = lib.vc_gene_joint_weighted(p(sblk), p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(W_d), 1, p(nuw_d), 0, noise, p(r_d),
                                        p(pm_d), p(pp_d), p(prior_d), p(Wt), R, Nc, p(start), 0, 1e-10, 40, *[p(many[k]) for k in names],
                                        stream)
        assert rc == 0, lib.vc_last_error(None)

    rows = []
    base = {"noise": "NegativeBinomial", "storage": "u16", "cells": Nc, "genes": Ng, "harmonics": H, "omega": omega, "board": board}
    for name, launch, out, nrows in (("vc_gene_joint", plain, one, 1), ("vc_gene_joint_weighted", weighted, many, R)):
        t = timed(launch, a.warmup, a.reps)
        it, st = out["it"].cpu().numpy(), out["st"].cpu().numpy()
        rows.append({"kernel": name, "start": "two-stage", "rows": nrows, **base, **t, "ms_per_row": t["ms_median"] / nrows,
                     "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)}, "steps_mean": float(it.mean()),
                     "steps_max": int(it.max()), "clamped_cells_per_pair": float(out["nc"].double().mean())})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = velocity_map_joint(S_host, U_host, xy, n_host, harmonics=H, **kw)
    fit_wall = time.perf_counter() - t0
    for tol_outer in (1e-8, 1e-6):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            t0 = time.perf_counter()
            bs = velocity_map_joint_bootstrap(S_host, U_host, xy, n_host, harmonics=H, **kw, n_boot=R, seed=0, fit=fit, tol_outer=tol_outer)
            wall = time.perf_counter() - t0
        st = np.asarray(bs.status)
        rows.append({"worker": "velocity_map_joint_bootstrap", "rows": R, "tol_outer": tol_outer, **base, "worker_wall_s": wall,
                     "velocity_map_joint_wall_s": fit_wall, "status": {s: int((st == s).sum()) for s in np.unique(st)},
                     "rounds_mean": float(bs.rounds.mean()), "rounds_max": int(bs.rounds.max()), "n_excluded_max": int(bs.n_excluded.max()),
                     "omega": float(fit.nu_omega[0, 0]), "laplace_std": float(fit.stds[0, 0]), "bootstrap_std": float(bs.stds[0, 0]),
                     "bootstrap_mean": float(bs.means[0, 0])})
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
