#!/usr/bin/env python
"""Times the kernel behind `gene_kinetics` / `velocity_map` (vc_gene_kinetics) with device events, after a warm-up, on a dense device
block of the bench generator's unspliced counts at the coefficients of a vc_gene_glm fit of its spliced counts, next to vc_gene_glm
itself in the same process; then `velocity_map` end to end by the wall clock (host counts in, host results out).

    python profiles/tools/time_gene_kinetics.py [--cells 50000] [--genes 2000] [--reps 5] [--warmup 2] [--omega 0.4] [--out FILE.json]

Prints one JSON line per timing: for uint16 / float32 storage the median, minimum and maximum of `reps` launches of each kernel (each
bracketed by its own pair of events), how the genes ended, the steps per gene and the passes over the cells (start + first point +
steps + 1 profile pass; refused trials not counted).  H = 1, NegativeBinomial at dispersion 0.3, NW = 1.  No GPU: it fails."""
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
from velocycle_amd.gene_harmonics import fourier_basis_from_directions        # noqa: E402
from velocycle_amd.gene_kinetics import DEFAULT_PRIOR, STATUS, velocity_map   # noqa: E402
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--omega", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gene_kinetics.py needs the GPU")
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
    nuw_d = torch.full((1,), a.omega, dtype=torch.float64, device=dev)
    prior_d = torch.tensor(DEFAULT_PRIOR, dtype=torch.float64, device=dev).expand(Ng, 4).contiguous()
    S32, U32 = S.T.contiguous(), U.T.contiguous()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)          # noqa: E731
    i32 = lambda: torch.empty(Ng, dtype=torch.int32, device=dev)                      # noqa: E731
    glm = dict(nu=f64(Ng, K), cov=f64(Ng, NH), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32())
    kin = dict(xy=f64(Ng, 2), cov=f64(Ng, 3), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32(), nc=i32(), score=f64(Ng, 1), info=f64(Ng, 1))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                            # noqa: E731
    rows = []
    for kind, sblk, ublk in ((_lib.VC_COUNTS_U16, u16_bits(S32), u16_bits(U32)), (_lib.VC_COUNTS_F32, S32, U32)):
        def launch_glm():
            rc = lib.vc_gene_glm(p(sblk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), _lib.NOISE["NegativeBinomial"], p(r_d), None, None, 1e-10,
                                 25, *[p(glm[k]) for k in ("nu", "cov", "ll", "dec", "it", "st")], stream)
            assert rc == 0, lib.vc_last_error(None)

        def launch_kin():
            rc = lib.vc_gene_kinetics(p(ublk), kind, Ng, Nc, Nc, p(B_d), K, p(logm_d), p(glm["nu"]), p(W_d), 1, p(nuw_d),
                                      _lib.NOISE["NegativeBinomial"], p(r_d), p(prior_d), None, 1e-10, 25,
                                      *[p(kin[k]) for k in ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")], stream)
            assert rc == 0, lib.vc_last_error(None)
        storage = "u16" if kind == _lib.VC_COUNTS_U16 else "f32"
        row = {"kernel": "vc_gene_glm", "noise": "NegativeBinomial", "storage": storage, "cells": Nc, "genes": Ng, "harmonics": H,
               **timed(launch_glm, a.warmup, a.reps), "steps_mean": float(glm["it"].float().mean()), "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
        t = timed(launch_kin, a.warmup, a.reps)
        it, st, nc = kin["it"].cpu().numpy(), kin["st"].cpu().numpy(), kin["nc"].cpu().numpy()
        passes = it + 3.0
        row = {"kernel": "vc_gene_kinetics", "noise": "NegativeBinomial", "storage": storage, "cells": Nc, "genes": Ng, "harmonics": H,
               "NW": 1, "omega": a.omega, **t, "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)},
               "steps_mean": float(it.mean()), "steps_max": int(it.max()), "passes_mean": float(passes.mean()),
               "ms_per_pass": t["ms_median"] / float(passes.mean()), "clamped_fraction": float(nc.sum() / (Nc * Ng)), "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
    # the outer fit end to end, once (host counts in, host results out), at the spliced fit's coefficients
    means = glm["nu"].T.cpu().numpy()
    U_host, n_host = U.cpu().numpy(), n.cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = velocity_map(U_host, xy, n_host, means, noisemodel="NegativeBinomial", dispersion=0.3)
    wall = time.perf_counter() - t0
    st = fit.kinetics.status
    row = {"worker": "velocity_map", "worker_wall_s": wall, "cells": Nc, "genes": Ng, "harmonics": H, "noise": "NegativeBinomial",
           "nu_omega": fit.nu_omega.reshape(-1).tolist(), "stds": fit.stds.reshape(-1).tolist(), "rounds": fit.rounds, "status": fit.status,
           "dec": fit.dec, "n_excluded": fit.n_excluded, "simulated_omega": list(sim["omegas"]),
           "gene_status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)},
           "clamped_fraction": float(fit.kinetics.n_clamped.sum() / (Nc * Ng)), "board": board}
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
