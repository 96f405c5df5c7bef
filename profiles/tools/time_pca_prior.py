#!/usr/bin/env python
"""Times the PCA phase prior (Phases.from_pca_heuristic) on the device against the host path, on one simulated layer.

    python profiles/tools/time_pca_prior.py [--cells 50000] [--genes 2000] [--reps 20] [--warmup 3] [--no-host] [--out FILE.json]

Prints one JSON line: staging (upload of the float32 layer in chunks + vc_pca_stage, wall clock, synchronised), the time of one
vc_pca_apply call (device events; median, minimum and maximum of `reps` calls after a warm-up) and the share of the 6.3 TB/s
achievable HBM rate that one read of the staged matrix in that time amounts to, the iteration count, the wall clock of the whole
from_pca_heuristic(device="cuda") call (median of three, after a first call that loads the library), and the wall clock of the host
path (np.log + sklearn's PCA, with whatever thread count the environment sets) on the same layer.  No GPU: it fails."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from velocycle_amd import phase_prior                     # noqa: E402
from velocycle_amd.anndata_lite import AnnDataLite        # noqa: E402
from velocycle_amd.containers import Phases               # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pca_prior.py needs the GPU")
    dev = torch.device("cuda:0")
    pr = torch.cuda.get_device_properties(dev)
    Nc, Ng = a.cells, a.genes
    S = simulate_counts(Nc=Nc, Ng=Ng, seed=21)["S"].numpy()
    tot = np.maximum(S.sum(1, dtype=np.float64), 1.0)
    v = (S / tot[:, None] * tot.mean()).astype(np.float32)
    del S
    ad = AnnDataLite(v, v)
    ad.layers["S_sz"] = v
    small = 1.0
    row = {"cells": Nc, "genes": Ng, "board": {"name": pr.name, "gcn_arch": getattr(pr, "gcnArchName", "")},
           "threads": {"torch": torch.get_num_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}}

    # first call: loads the library, creates the context
    Phases.from_pca_heuristic(AnnDataLite(v[:256], v[:256]), layer="spliced", small_count=small, device=dev)
    totals = []
    for _ in range(3):
        t, p = wall(lambda: Phases.from_pca_heuristic(ad, layer="S_sz", small_count=small, device=dev))
        totals.append(t)
    row.update(device_total_s=float(np.median(totals)), device_total_all_s=totals, n_iter=p.pca.n_iter_, residual=p.pca.residual_,
               converged=p.pca.converged_)

    # the parts
    step = phase_prior.default_chunk_cells(Ng)

    def stage():
        ops = phase_prior._HipOps(Nc, Ng, dev)
        for c0 in range(0, Nc, step):
            blk = phase_prior._dense_block(v, c0, min(Nc, c0 + step), Ng, dev)
            ops.stage(blk, c0, small)
        return ops
    stage_s = []
    for _ in range(3):
        t, ops = wall(stage)
        stage_s.append(t)
    row.update(stage_s=float(np.median(stage_s)), stage_all_s=stage_s, chunk_cells=step)
    ops.set_mean((ops.colsum.cpu() / Nc).to(torch.float32))
    Q = torch.linalg.qr(torch.randn((Ng, 8), dtype=torch.float64))[0].to(torch.float32).contiguous().to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        rc = ops.lib.vc_pca_apply(C.c_void_p(ops.X.data_ptr()), Nc, Ng, Ng, C.c_void_p(ops.mu.data_ptr()), C.c_void_p(Q.data_ptr()),
                                  C.c_void_p(ops.Y.data_ptr()), C.c_void_p(ops.Z.data_ptr()), C.c_void_p(ops.ws.data_ptr()),
                                  ops.ws.numel(), 0, stream)
        assert rc == 0, ops.lib.vc_last_error(None)
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
    med = float(np.median(ms))
    row.update(apply_ms_median=med, apply_ms_min=float(np.min(ms)), apply_ms_max=float(np.max(ms)), reps=a.reps, warmup=a.warmup,
               matrix_bytes=4 * Nc * Ng, share_of_achievable_hbm=4 * Nc * Ng / (med * 1e-3) / HBM_ACHIEVABLE)
    _, (Y, Z) = wall(lambda: ops.apply(Q.cpu()))
    t_iter, _ = wall(lambda: ops.apply(Q.cpu()))
    row.update(apply_with_transfers_s=t_iter)
    del ops

    if not a.no_host:
        host = []
        for _ in range(2):
            t0 = time.perf_counter()
            h = Phases.from_pca_heuristic(ad, layer="S_sz", small_count=small)
            host.append(time.perf_counter() - t0)
        d = np.abs(np.abs(np.sum(h.phi_xy.values * p.phi_xy.values, 0)) - 1.0)
        row.update(host_total_s=float(np.min(host)), host_all_s=host, host_solver=str(getattr(h.pca, "_fit_svd_solver", "")),
                   device_over_host=row["device_total_s"] / float(np.min(host)), median_1_minus_cos_between_priors=float(np.median(d)))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
