#!/usr/bin/env python
"""Times the predictive PIT (velocycle_amd.predictive.predictive_pit -> vc_predictive_pit) with device events.

    python profiles/tools/time_pit.py [--case vjoint_3000x200] [--draws 50] [--bins 20] [--reps 5] [--out FILE.json]

The problem is a case of tests/golden/make_oracle_fits.py at its initial parameters (the size profiles/r11_draw_model.md timed
vc_pointwise_density and vc_predictive_check at), `draws` guide samples made on the device, shape_inv handed over once.  Two figures,
three untimed calls before `reps` timed ones each: one pair of events around ONE library call (all cells, tables zeroed outside the
pair, no dense output: the histogram constants and the element kernel), and around one call of predictive_pit (allocation and
zeroing of the tables, the library call, the copies to the host).  Prints one JSON line.  No GPU: it fails, it does not fall back."""
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
    ap.add_argument("--draws", type=int, default=50)
    ap.add_argument("--bins", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pit.py needs the GPU")
    dev = torch.device("cuda:0")
    spec = make_spec(a.case)
    eng = HipEngine(spec, device=dev)
    eng.init_params()
    vel = spec.kind == "velocity"
    names = ["ν", "ϕxy"] + (["shape_inv"] if spec.noisemodel == "NegativeBinomial" else []) + (["logγg", "logβg", "νω"] if vel else [])
    draws = eng.sample_posterior(names, a.draws, seed=11)
    draws = {k: (v[:1].contiguous() if k == "shape_inv" else v) for k, v in draws.items()}
    D, nm, Ng, Nc, B = a.draws, 2 if vel else 1, spec.Ng, eng.Nc_local, a.bins
    ptr, stride, keep = P._device_draws(eng, draws, D)
    gene = torch.zeros((nm, Ng, B), dtype=torch.int64, device=dev)
    cell = torch.zeros((nm, Nc, B), dtype=torch.int64, device=dev)
    g = lambda k: ptr.get(k)

    def library_call():
        eng._check(eng.lib.vc_predictive_pit(
            eng._h, C.c_int64(D), g("ϕxy"), C.c_int64(stride["ϕxy"]), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"), g("logγg"),
            C.c_int64(stride.get("logγg", 0)), g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"), C.c_int64(stride.get("νω", 0)),
            C.c_uint64(7), C.c_int32(B), C.c_int64(0), C.c_int64(Nc), C.c_void_p(gene.data_ptr()), C.c_void_p(cell.data_ptr()), None,
            eng._stream()))
    lib_ms = events(library_call, a.reps)
    torch.cuda.synchronize()
    py_ms = events(lambda: P.predictive_pit(eng, draws, seed=7, bins=B), a.reps)
    rec = P.predictive_pit(eng, draws, seed=7, bins=B)
    S = spec.S.numpy()
    row = {"case": a.case, "cells": Nc, "genes": Ng, "draws": D, "bins": B, "matrices": nm, "count_storage": eng.stats["count_storage"],
           "library_call_ms": [round(x, 4) for x in lib_ms], "library_call_ms_median": float(np.median(lib_ms)),
           "predictive_pit_ms": [round(x, 4) for x in py_ms], "predictive_pit_ms_median": float(np.median(py_ms)),
           "zero_share_S": float((S == 0).mean()), "max_count_S": float(S.max()),
           "pooled": {m: {k: (v if k != "hist" else v.tolist()) for k, v in p.items()} for m, p in rec.pooled().items()}}
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
