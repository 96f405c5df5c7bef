#!/usr/bin/env python
"""Times the kernel behind the cell bootstrap of the batch-aware harmonic fit (vc_gene_glm_batch_weighted, R rows of Poisson(1) case
weights, warm-started from the full-data fit, no covariances) next to vc_gene_glm_batch and vc_gene_glm_weighted on the same dense
device block, in one run on one board, with device events after a warm-up; and the worker
`velocycle_amd.gene_bootstrap.gene_harmonics_batched_bootstrap` end to end (host counts in, host replicates out: staging, the
unweighted fit, the weight draws, the replicates) by the wall clock.

    python profiles/tools/time_gene_batch_bootstrap.py [--cells 50000] [--genes 2000] [--harmonics 1] [--batches 4] [--rows 200]
                                                       [--reps 3] [--warmup 1] [--no-worker] [--out FILE.json]

Negative binomial, uint16 counts, batches of equal size with the cells in batch order.  One JSON line per kernel: median, minimum and
maximum of `reps` launches (each bracketed by its own pair of events), how the (gene, row) pairs ended, the steps, the passes per
replicate (mean steps + 1) and the time per pass and row.  No GPU: it fails, it does not fall back."""
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
from velocycle_amd.gene_bootstrap import draw_weights, gene_harmonics_batched_bootstrap               # noqa: E402
from velocycle_amd.gene_harmonics import STATUS, fourier_basis_from_directions                        # noqa: E402
from velocycle_amd.simulate import simulate_counts        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--harmonics", type=int, default=1)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-worker", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gene_batch_bootstrap.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda")
    pr = torch.cuda.get_device_properties(dev)
    board = {"name": pr.name, "uuid": str(getattr(pr, "uuid", "")), "gcn_arch": getattr(pr, "gcnArchName", "")}
    Nc, H, R, Nb = a.cells, a.harmonics, a.rows, a.batches
    K, NH = 2 * H + 1, (2 * H + 1) * (H + 1)
    sim = simulate_counts(Nc=Nc, Ng=a.genes, seed=21, device=dev)
    S = sim["S"]
    S = S[:, S.sum(0) > 0].contiguous()
    Ng = int(S.shape[1])
    n = S.sum(1).clamp_min(1.0).double()
    phis = sim["phis"].double().cpu().numpy()
    xy = np.stack([np.cos(phis), np.sin(phis)])
    bounds = [Nc * b // Nb for b in range(Nb + 1)]
    labels = np.repeat(np.arange(Nb), np.diff(bounds))
    seg = (C.c_int64 * (Nb + 1))(*bounds)
    B_d = fourier_basis_from_directions(xy, H).float().to(dev).contiguous()
    logm_d = torch.log(n).float().contiguous()
    r_d = torch.full((Ng,), 1.0 / 0.3, dtype=torch.float32, device=dev)
    dm_d = torch.zeros((Ng, Nb), dtype=torch.float64, device=dev)
    dq_d = torch.full((Ng, Nb), 4.0, dtype=torch.float64, device=dev)                                  # std 0.5
    i = S.T.contiguous().to(torch.int32)
    i[i >= 32768] -= 65536
    blk = i.to(torch.int16)
    del i
    W_d = draw_weights(R, Nc, 0, dev)
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)                                   # noqa: E731
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)                                     # noqa: E731
    one = dict(nu=f64(Ng, K), delta=f64(Ng, Nb), cov=f64(Ng, NH), dvar=f64(Ng, Nb), ll=f64(Ng), dec=f64(Ng), it=i32(Ng), st=i32(Ng))
    many = dict(nu=f64(R, Ng, K), delta=f64(R, Ng, Nb), ll=f64(R, Ng), dec=f64(R, Ng), it=i32(R, Ng), st=i32(R, Ng))
    single = dict(nu=f64(R, Ng, K), ll=f64(R, Ng), dec=f64(R, Ng), it=i32(R, Ng), st=i32(R, Ng))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                                             # noqa: E731
    noise = _lib.NOISE["NegativeBinomial"]
    head = (p(blk), _lib.VC_COUNTS_U16, Ng, Nc, Nc, p(B_d), K, p(logm_d), noise, p(r_d))

    def batch():
        rc = lib.vc_gene_glm_batch(*head, Nb, seg, p(dm_d), p(dq_d), None, None, 1e-10, 25,
                                   *[p(one[k]) for k in ("nu", "delta", "cov", "dvar", "ll", "dec", "it", "st")], stream)
        assert rc == 0, lib.vc_last_error(None)

    def weighted():                                        # no offsets: warm-started from the nu `batch` left in one["nu"]
        rc = lib.vc_gene_glm_weighted(*head, None, None, p(W_d), R, Nc, p(one["nu"]), 1e-10, 25, p(single["nu"]), None, p(single["ll"]),
                                      p(single["dec"]), p(single["it"]), p(single["st"]), stream)
        assert rc == 0, lib.vc_last_error(None)

    def batch_weighted():                                  # warm-started from the full-data fit of `batch`; no covariances
        rc = lib.vc_gene_glm_batch_weighted(*head, Nb, seg, p(dm_d), p(dq_d), None, None, p(W_d), R, Nc, p(one["nu"]), p(one["delta"]),
                                            1e-10, 25, p(many["nu"]), p(many["delta"]), None, None, p(many["ll"]), p(many["dec"]),
                                            p(many["it"]), p(many["st"]), stream)
        assert rc == 0, lib.vc_last_error(None)

    rows = []
    for name, launch, out, nrows in (("vc_gene_glm_batch", batch, one, 1), ("vc_gene_glm_weighted", weighted, single, R),
                                     ("vc_gene_glm_batch_weighted", batch_weighted, many, R)):
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
        passes = float(it.mean()) + 1
        row = {"kernel": name, "noise": "NegativeBinomial", "storage": "u16", "cells": Nc, "genes": Ng, "harmonics": H, "batches": Nb,
               "rows": nrows, "warm_start": name.endswith("weighted"), "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
               "ms_max": float(np.max(ms)), "reps": a.reps, "warmup": a.warmup,
               "status": {STATUS[int(s)]: int((st == s).sum()) for s in np.unique(st)}, "steps_mean": float(it.mean()),
               "steps_max": int(it.max()), "passes_per_replicate": passes, "ms_per_pass_and_row": float(np.median(ms)) / (passes * nrows),
               "board": board}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if not a.no_worker:                                    # the worker end to end, once (host counts in, host replicates out)
        S_host = S.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bs = gene_harmonics_batched_bootstrap(S_host, xy, n.cpu().numpy(), labels, harmonics=H, noisemodel="NegativeBinomial",
                                              dispersion=0.3, n_boot=R, seed=0)
        wall = time.perf_counter() - t0
        ratio = bs.stds / bs.fit.stds
        row = {"worker_wall_s": wall, "cells": Nc, "genes": Ng, "harmonics": H, "batches": Nb, "rows": R, "noise": "NegativeBinomial",
               "ok_share": float(bs.ok.mean()), "median_std_boot_over_std_hess": [float(v) for v in np.nanmedian(ratio, axis=1)],
               "median_delta_std_boot_over_std_hess": [float(v) for v in np.nanmedian(bs.delta_nu_stds / bs.fit.delta_nu_stds, axis=1)],
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
