#!/usr/bin/env python
"""Times the pointwise predictive density (velocycle_amd.predictive.pointwise_density -> vc_pointwise_density) with device events.

    python profiles/tools/time_pointwise.py [--cells 50000] [--genes 2000] [--draws 500] [--reps 5] [--configs vjoint,vcond] [--out FILE.json]

Per configuration -- "vjoint": mean-field velocity model, nothing conditioned, negative binomial (S and U per draw); "vcond": the
tutorials' conditioning (phases, nu, shape_inv fixed: S evaluated once, U per draw) -- it draws `draws` guide samples on the device
(vc_sample_posterior at the initial parameters), makes one warm-up call and `reps` timed ones (one pair of events around each call of
pointwise_density: the library's launches plus the host side's pointer set-up, in one process), and prints one JSON line: median /
minimum / maximum milliseconds, element-draws per second, and the time the instruction list of the draw loop would need when
issued alone: a wave64 float32 VALU instruction 4 cycles, a transcendental 16 (quarter rate), on 1 024 SIMDs at the clock
profiles/valu_model.json records for the likelihood kernel's mix (`mix_clock_ghz`).  `--valu` / `--trans`: instructions per
element-draw counted from the emitted ISA, one value per configuration in the order of `--configs` (e.g. --valu 44.8,44.8).
`--cpu-checker` adds the float32 checker of tests/pointwise_checker.py on the CPU at 3 000 x 200 x 50, scaled by element-draws.
No GPU: it fails, it does not fall back."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from velocycle_amd.engine import HipEngine                    # noqa: E402
from velocycle_amd.predictive import pointwise_density        # noqa: E402
from velocycle_amd.workloads import make_velocity_spec        # noqa: E402

SIMDS = 1024
CLOCK_GHZ = float(json.load(open(os.path.join(ROOT, "profiles", "valu_model.json")))["mix_clock_ghz"])
NS_PER_WAVE_VALU = 4 / CLOCK_GHZ    # one wave64 float32 VALU instruction on a SIMD-16: 4 cycles
NS_PER_WAVE_TRANS = 16 / CLOCK_GHZ  # transcendental unit: quarter rate
SITES = ["ν", "ϕxy", "shape_inv", "logγg", "logβg", "νω"]


def time_config(mode, a, dev, valu, trans):
    spec = make_velocity_spec(Nc=a.cells, Ng=a.genes, mode=mode, seed=3)
    eng = HipEngine(spec, device=dev)
    eng.init_params(torch.full((spec.Ng + spec.Nx * spec.Nhw, spec.rho_rank), 0.02) if spec.guide == "lrmn" else None)
    draws = eng.sample_posterior(SITES, a.draws, seed=11)
    # conditioned / Delta sites once, as the fit driver hands them over
    draws = {k: (v[:1].contiguous() if (k in spec.condition_on or k == "shape_inv") else v) for k, v in draws.items()}
    torch.cuda.synchronize()
    rec = pointwise_density(eng, draws)               # warm-up (allocates the engine's workspaces)
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rec = pointwise_density(eng, draws)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    mats_per_draw = 1 if mode.startswith("vcond") else 2
    ed = a.cells * a.genes * a.draws
    floor_ms = ed / 64 * (valu * NS_PER_WAVE_VALU + trans * NS_PER_WAVE_TRANS) / SIMDS * 1e-6 if valu else None
    row = {"config": mode, "cells": a.cells, "genes": a.genes, "draws": a.draws, "matrices_per_draw": mats_per_draw,
           "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)), "reps": a.reps,
           "element_draws_per_s": ed / (float(np.median(ms)) * 1e-3), "valu_per_element_draw": valu, "trans_per_element_draw": trans, "clock_ghz": CLOCK_GHZ,
           "issue_floor_ms": floor_ms, "share_of_issue_floor": (floor_ms / float(np.median(ms))) if floor_ms else None,
           "elpd_waic": rec.elpd_waic, "count_storage": eng.stats["count_storage"]}
    eng.close()
    return row


def cpu_checker_seconds():
    from tests import pointwise_checker as PC
    sp = make_velocity_spec(Nc=3000, Ng=200, mode="vjoint", seed=3)
    g = torch.Generator().manual_seed(1)
    D = 50
    z = {"in_kind": "velocity", "in_noisemodel": "NegativeBinomial", "in_H": 1, "in_Hw": 1, "in_S": sp.S.numpy(), "in_U": sp.U.numpy(),
         "in_count_factor": sp.count_factor.numpy(), "in_with_delta_nu": False, "in_D": sp.D.numpy(),
         "draw_ν": (sp.mu_nu[None] + 0.03 * torch.randn((D,) + tuple(sp.mu_nu.shape), generator=g)).numpy(),
         "draw_ϕxy": (sp.phixy_prior[None] + torch.randn((D,) + tuple(sp.phixy_prior.shape), generator=g)).numpy(),
         "draw_shape_inv": np.full((1, sp.Ng), 0.5, dtype=np.float32), "draw_logγg": torch.zeros(D, sp.Ng).numpy(),
         "draw_logβg": torch.full((D, sp.Ng), 2.0).numpy(), "draw_νω": (0.3 + torch.zeros(D, sp.Nx, sp.Nhw)).numpy()}
    t0 = time.perf_counter()
    PC.evaluate(z, torch.float32)
    return time.perf_counter() - t0, 3000 * 200 * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="vjoint,vcond")
    ap.add_argument("--valu", default="", help="VALU instructions per element-draw (from the ISA) without the transcendentals, per configuration")
    ap.add_argument("--trans", default="", help="transcendental instructions per element-draw (from the ISA), per configuration")
    ap.add_argument("--cpu-checker", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pointwise.py needs the GPU")
    dev = torch.device("cuda:0")
    rows = []
    modes = a.configs.split(",")
    per = lambda txt: [float(x) for x in txt.split(",")] if txt else [0.0] * len(modes)
    valu, trans = per(a.valu), per(a.trans)
    if len(valu) != len(modes) or len(trans) != len(modes):
        raise SystemExit("--valu / --trans need one value per configuration")
    for mode, v, t in zip(modes, valu, trans):
        rows.append(time_config(mode, a, dev, v, t))
        print(json.dumps(rows[-1]), flush=True)
    if a.cpu_checker:
        s, ed = cpu_checker_seconds()
        rows.append({"config": "cpu_float32_checker_3000x200x50", "seconds": s, "element_draws": ed,
                     "scaled_to_request_s": s * (a.cells * a.genes * a.draws) / ed})
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
