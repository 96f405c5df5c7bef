#!/usr/bin/env python
"""Times the Python calls velocycle_amd.predictive.predictive_check (-> vc_predictive_check) and, as context at the same sizes in the
same process, predictive.pointwise_density (-> vc_pointwise_density), with device events.

    python profiles/tools/time_ppc.py [--sizes 3000x200,50000x2000] [--draws 50] [--reps 5] [--regions 3] [--out FILE.json]

Per size: the V-joint negative-binomial velocity model (S and U replicated per draw) at its initial parameters, `draws` guide
samples made on the device.  The clock is warmed by two untimed calls; then `regions` regions of `reps` calls each, one pair of events
per call.  The timed region is the WHOLE Python call, not the library call alone: allocating and zeroing the output tensors, the
comparison that recognises a site repeated over the draws, the library's launches, the synchronisation the call owes its status
latch, and the copies of the tables to the host.  The rows are labelled by the Python call for that reason.
Prints one JSON line per size and call: median / minimum / maximum milliseconds over all timed calls, the medians of the regions,
replicates per second, the board (`torch.cuda.get_device_properties` name and uuid where available).  No GPU: it fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from velocycle_amd.engine import HipEngine                                       # noqa: E402
from velocycle_amd.predictive import pointwise_density, predictive_check       # noqa: E402
from velocycle_amd.workloads import make_velocity_spec                          # noqa: E402

SITES = ["ν", "ϕxy", "shape_inv", "logγg", "logβg", "νω"]


def timed(fn, reps, regions):
    fn(), fn()
    out = []
    for _ in range(regions):
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out.append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3000x200,50000x2000")
    ap.add_argument("--draws", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ppc.py needs the GPU")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    board = {"name": prop.name, "uuid": str(getattr(prop, "uuid", ""))}
    rows = []
    for size in a.sizes.split(","):
        nc, ng = (int(x) for x in size.split("x"))
        spec = make_velocity_spec(Nc=nc, Ng=ng, mode="vjoint", seed=3)
        eng = HipEngine(spec, device=dev)
        eng.init_params()
        draws = eng.sample_posterior(SITES, a.draws, seed=11)
        draws = {k: (v[:1].contiguous() if k == "shape_inv" else v) for k, v in draws.items()}
        torch.cuda.synchronize()
        for name, fn in (("predictive.predictive_check", lambda: predictive_check(eng, draws, seed=5)),
                         ("predictive.pointwise_density", lambda: pointwise_density(eng, draws))):
            reg = timed(fn, a.reps, a.regions)
            flat = [x for r in reg for x in r]
            n = 2 * nc * ng * a.draws
            rows.append({"python_call": name, "cells": nc, "genes": ng, "draws": a.draws, "ms_median": float(np.median(flat)),
                         "ms_min": float(np.min(flat)), "ms_max": float(np.max(flat)), "region_medians_ms": [float(np.median(r)) for r in reg],
                         "reps": a.reps, "regions": a.regions, "element_draws_per_s": n / (float(np.median(flat)) * 1e-3),
                         "clock_mhz_after": eng.device_clock_mhz(), "board": board, "count_storage": eng.stats["count_storage"]})
            print(json.dumps(rows[-1]), flush=True)
        eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
