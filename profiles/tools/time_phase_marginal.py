#!/usr/bin/env python
"""Times phase-marginal scoring (velocycle_amd.predictive.phase_marginal -> vc_phase_marginal) with device events.

    python profiles/tools/time_phase_marginal.py [--case vjoint_3000x200] [--draws 16] [--bins 128] [--reps 5] [--out FILE.json]

The problem is a case of tests/golden/make_oracle_fits.py at its initial parameters (the size profiles/r11_draw_model.md and
profiles/r12_pit.md timed the neighbours at), `draws` guide samples of the gene-level and global sites made on the device, shape_inv
handed over once, the flat prior.  Two figures, three untimed calls before `reps` timed ones each: one pair of events around ONE
library call (all cells, posterior written, no per-draw output: the histogram constants and the kernel), and around one call of
phase_marginal (allocation, the model prior's table, the library call, the copies to the host).  Prints one JSON line with
evaluations = cells x genes x matrices x bins x draws and the time per evaluation.  No GPU: it fails, it does not fall back."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden.make_oracle_fits import make_spec           # noqa: E402
from velocycle_amd import predictive as P                     # noqa: E402
from velocycle_amd.engine import HipEngine                    # noqa: E402


def events(fn, reps):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="vjoint_3000x200")
    ap.add_argument("--draws", type=int, default=16)
    ap.add_argument("--bins", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_phase_marginal.py needs the GPU")
    dev = torch.device("cuda:0")
    spec = make_spec(a.case)
    eng = HipEngine(spec, device=dev)
    eng.init_params()
    vel = spec.kind == "velocity"
    names = ["ν"] + (["shape_inv"] if spec.noisemodel == "NegativeBinomial" else []) + (["logγg", "logβg", "νω"] if vel else []) + \
        (["Δν"] if spec.with_delta_nu and spec.Nb > 0 else [])
    draws = eng.sample_posterior(names, a.draws, seed=11)
    draws = {k: (v[:1].contiguous() if k in ("shape_inv", "Δν") else v) for k, v in draws.items()}
    D, nm, Ng, Nc, B = a.draws, 2 if vel else 1, spec.Ng, eng.Nc_local, a.bins
    ptr, stride, keep = P._device_draws(eng, draws, D, phixy=False)
    evidence = torch.empty((Nc,), dtype=torch.float64, device=dev)
    post = torch.empty((Nc, B), dtype=torch.float32, device=dev)
    g = lambda k: ptr.get(k)

    def library_call():
        eng._check(eng.lib.vc_phase_marginal(
            eng._h, C.c_int64(D), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"), g("logγg"), C.c_int64(stride.get("logγg", 0)),
            g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"), C.c_int64(stride.get("νω", 0)), C.c_int32(B), None, C.c_int64(0),
            C.c_int64(Nc), C.c_void_p(evidence.data_ptr()), C.c_void_p(post.data_ptr()), None, eng._stream()))
    lib_ms = events(library_call, a.reps)
    torch.cuda.synchronize()
    py_ms = events(lambda: P.phase_marginal(eng, draws, bins=B), a.reps)
    rec = P.phase_marginal(eng, draws, bins=B, phase_prior="flat")
    evals = Nc * Ng * nm * B * D
    med = float(np.median(lib_ms))
    row = {"case": a.case, "cells": Nc, "genes": Ng, "draws": D, "bins": B, "matrices": nm, "count_storage": eng.stats["count_storage"],
           "nu_given_once": stride["ν"] == 0, "evaluations": evals,
           "library_call_ms": [round(x, 4) for x in lib_ms], "library_call_ms_median": med, "ns_per_evaluation": med * 1e6 / evals,
           "phase_marginal_ms": [round(x, 4) for x in py_ms], "phase_marginal_ms_median": float(np.median(py_ms)),
           "elpd_flat": rec.elpd, "mean_entropy": float(rec.entropy.mean()), "mean_resultant_length": float(rec.resultant_length.mean())}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
