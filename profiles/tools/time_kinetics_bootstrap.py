#!/usr/bin/env python
"""Times the kernel behind the cell bootstrap of the kinetics fit (vc_gene_kinetics_weighted, R rows of Poisson(1) case weights,
warm-started from the unweighted fit, no covariances) next to vc_gene_kinetics on the same dense device block, in one run on one board,
with device events after a warm-up; then `velocity_map` and `velocycle_amd.kinetics_bootstrap.velocity_map_bootstrap` end to end by the
wall clock (host counts in, host replicates out: staging, the weight draws, the weighted constants, the outer iteration of all rows).

    python profiles/tools/time_kinetics_bootstrap.py [--cells 50000] [--genes 2000] [--rows 200] [--omega 0.4] [--reps 3] [--warmup 1]
                                                     [--no-worker] [--out FILE.json]

The bench generator's unspliced counts at the coefficients of a vc_gene_glm fit of its spliced counts, H = 1, NegativeBinomial at
dispersion 0.3, NW = 1, uint16 counts.  One JSON line per kernel: median, minimum and maximum of `reps` launches (each bracketed by its
own pair of events), how the (gene, row) pairs ended, the steps, the passes over the cells per pair (start + first point + steps + 1
profile pass; refused trials not counted) and the time per pass and row.  No GPU: it fails, it does not fall back."""
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
from velocycle_amd.gene_bootstrap import draw_weights     # noqa: E402
from velocycle_amd.gene_harmonics import fourier_basis_from_directions        # noqa: E402
from velocycle_amd.gene_kinetics import DEFAULT_PRIOR, STATUS, velocity_map   # noqa: E402
from velocycle_amd.kinetics_bootstrap import velocity_map_bootstrap           # noqa: E402
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
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--omega", type=float, default=0.4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-worker", action="store_true")
    ap.add_argument("--tol-outer", type=float, nargs="+", default=[1e-8, 1e-6])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_kinetics_bootstrap.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, H, K, NH, R = a.cells, 1, 3, 6, a.rows
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
    nuw_d = torch.full((1,), a.omega, dtype=torch.float64, device=dev)
    prior_d = torch.tensor(DEFAULT_PRIOR, dtype=torch.float64, device=dev).expand(Ng, 4).contiguous()
    sblk, ublk = u16_bits(S.T.contiguous()), u16_bits(U.T.contiguous())
    Wt_d = draw_weights(R, Nc, 0, dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)            # noqa: E731
    glm = dict(nu=f64(Ng, K), cov=f64(Ng, NH), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng))
    kin = dict(xy=f64(Ng, 2), cov=f64(Ng, 3), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng), nc=i32(Ng), score=f64(Ng, 1), info=f64(Ng, 1))
    many = dict(xy=f64(R, Ng, 2), ll=f64(R, Ng), dec=f64(R, Ng), it=i32(R, Ng), st=i32(R, Ng), nc=i32(R, Ng), score=f64(R, Ng, 1),
                info=f64(R, Ng, 1))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    kind, noise = _lib.VC_COUNTS_U16, _lib.NOISE["NegativeBinomial"]
    rc = lib.vc_gene_glm(p(sblk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d), None, None, 1e-10, 25,
                         *[p(glm[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
    assert rc == 0, lib.vc_last_error(None)

    def plain():
        rc = lib.vc_gene_kinetics(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(W_d), 1, p(nuw_d), noise, p(r_d),
                                  p(prior_d), None, 1e-10, 25,
                                  *[p(kin[k]) for k in ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")], stream)
        assert rc == 0, lib.vc_last_error(None)

    def weighted():                                        # warm-started at the (x, y) `plain` left in kin["xy"]; no covariances
        rc = lib.vc_gene_kinetics_weighted(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), 0, p(W_d), 1, p(nuw_d), 0, noise,
                                           p(r_d), p(prior_d), p(Wt_d), R, Nc, p(kin["xy"]), 0, 1e-10, 25, p(many["xy"]), None,
                                           *[p(many[k]) for k in ("ll", "dec", "it", "st", "nc", "score", "info")], stream)
        assert rc == 0, lib.vc_last_error(None)

    rows = []
    for name, launch, out, nrows in (("vc_gene_kinetics", plain, kin, 1), ("vc_gene_kinetics_weighted", weighted, many, R)):
        t = timed(launch, a.warmup, a.reps)
        it, st = out["it"].cpu().numpy(), out["st"].cpu().numpy()
        passes = float(it.mean()) + 3.0
        row = {"kernel": name, "noise": "NegativeBinomial", "storage": "u16", "cells": Nc, "genes": Ng, "harmonics": H, "NW": 1,
               "omega": a.omega, "rows": nrows, "warm_start": nrows > 1, "grid": "row fastest" if nrows > 1 else "genes", **t,
               "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)}, "steps_mean": float(it.mean()),
               "steps_max": int(it.max()), "passes_mean": passes, "ms_per_pass_and_row": t["ms_median"] / (passes * nrows), "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if not a.no_worker:                                    # the workers end to end, once each (host counts in, host results out)
        means = glm["nu"].T.cpu().numpy()
        U_host, n_host = U.cpu().numpy(), n.cpu().numpy()
        kw = dict(noisemodel="NegativeBinomial", dispersion=0.3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = velocity_map(U_host, xy, n_host, means, **kw)
        map_wall = time.perf_counter() - t0
        for tol_outer in a.tol_outer:                      # the default, and what the float32 sums resolve at this size
            t1 = time.perf_counter()
            bs = velocity_map_bootstrap(U_host, xy, n_host, means, **kw, n_boot=R, seed=0, fit=fit, tol_outer=tol_outer)
            t2 = time.perf_counter()
            names, counts = np.unique(bs.status, return_counts=True)
            late = bs.dec[~bs.ok]
            row = {"worker": "velocity_map_bootstrap", "tol_outer": tol_outer, "worker_wall_s": t2 - t1, "velocity_map_wall_s": map_wall,
                   "cells": Nc, "genes": Ng, "harmonics": H, "rows": R, "noise": "NegativeBinomial",
                   "nu_omega": fit.nu_omega.reshape(-1).tolist(), "laplace_std": fit.stds.reshape(-1).tolist(), "fit_dec": fit.dec,
                   "bootstrap_std_ok": bs.stds.reshape(-1).tolist(), "bootstrap_mean_ok": bs.means.reshape(-1).tolist(),
                   "bootstrap_std_all_rows": bs.nu_omega_replicates.std(0, ddof=1).reshape(-1).tolist(),
                   "status": {str(k): int(v) for k, v in zip(names, counts)}, "rounds_mean": float(bs.rounds.mean()),
                   "rounds_max": int(bs.rounds.max()), "dec_of_the_rows_not_converged_min_median_max":
                   [float(np.min(late)), float(np.median(late)), float(np.max(late))] if len(late) else None,
                   "n_excluded_max": int(bs.n_excluded.max()), "fit_rounds": fit.rounds, "fit_n_excluded": fit.n_excluded, "board": board}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
