"""Pointwise predictive density of a fit over posterior draws: lppd, its WAIC penalty, their sums per gene and per cell.

For every observed count the likelihood is averaged over D guide draws (`lppd`), the variance over the draws of its logarithm is the
WAIC penalty (`p_waic`); `elpd_waic = lppd - p_waic` is what two fits of the same data are compared by (`compare`).  The reference
has no function for this; the model whose log-probabilities are taken is the reference's (velocity_inference_model.py:338-386,
phase_inference_model.py:343-395).  Every number comes from one HIP kernel (vc_pointwise_density, csrc/vc_pointwise.hip) that walks
draws x genes x cells on the engine's own copy of the counts; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

MAX_POINTWISE_BYTES = 1 << 30        # the dense per-element lppd (float32, per matrix and rank) is refused above this size
CELL_ALIGN = 64                      # calls cut the cells at multiples of this (one workgroup of the kernel)
QUANTITIES = ("lppd", "mean", "p_waic")


@dataclass
class PredictiveDensity:
    """Sums over cells (`*_gene`, (Ng,)) and over genes (`*_cell`, (Nc,)) per count matrix {"S": ..., "U": ...}, float64 CPU tensors."""
    lppd_gene: Dict[str, torch.Tensor]
    lppd_cell: Dict[str, torch.Tensor]
    mean_gene: Dict[str, torch.Tensor]
    mean_cell: Dict[str, torch.Tensor]
    p_waic_gene: Dict[str, torch.Tensor]
    p_waic_cell: Dict[str, torch.Tensor]
    n_draws: int
    pointwise: Optional[Dict[str, torch.Tensor]] = None      # {"S": (Ng, Nc) float32 lppd per element, ...} when asked for

    @staticmethod
    def _diff(a, b):
        return {m: a[m] - b[m] for m in a}

    @property
    def elpd_waic_gene(self):
        return self._diff(self.lppd_gene, self.p_waic_gene)

    @property
    def elpd_waic_cell(self):
        return self._diff(self.lppd_cell, self.p_waic_cell)

    @property
    def lppd(self) -> float:
        return float(sum(v.sum() for v in self.lppd_cell.values()))

    @property
    def p_waic(self) -> float:
        return float(sum(v.sum() for v in self.p_waic_cell.values()))

    @property
    def elpd_waic(self) -> float:
        return self.lppd - self.p_waic

    @property
    def waic(self) -> float:
        return -2.0 * self.elpd_waic


def check_request(noisemodel: str, n_draws: int, Ng: int, Nc: int, n_matrices: int, return_pointwise: bool):
    """The refusals that need no device: raised before any library or GPU call."""
    if noisemodel == "Lognormal":
        raise NotImplementedError("pointwise_density: Lognormal noise is not supported (NegativeBinomial or Poisson)")
    if noisemodel not in ("NegativeBinomial", "Poisson"):
        raise ValueError(f"{noisemodel} not allowed")
    if int(n_draws) < 2:
        raise ValueError(f"pointwise_density needs at least 2 draws (the variance over draws divides by n - 1), got {n_draws}")
    if return_pointwise and 4 * int(Ng) * int(Nc) * int(n_matrices) > MAX_POINTWISE_BYTES:
        raise ValueError(f"return_pointwise: the dense lppd of {n_matrices} x {Ng} x {Nc} elements exceeds {MAX_POINTWISE_BYTES} bytes; "
                         "use the per-gene / per-cell sums")


def _draw_count(draws) -> int:
    if "ν" not in draws or "ϕxy" not in draws:
        raise ValueError("draws must hold at least the sites 'ν' and 'ϕxy' (what HipEngine.sample_posterior returns)")
    # a site that is the same in every draw may be given once: the number of draws is the longest leading dimension
    return max(int(draws[k].shape[0]) for k in ("ν", "ϕxy", "logγg", "logβg", "νω") if k in draws)


def pointwise_density(engine, draws: Dict[str, torch.Tensor], *, return_pointwise: bool = False,
                      chunk_cells: Optional[int] = None) -> PredictiveDensity:
    """lppd / mean / p_waic of this engine's cells under explicit draws.

    draws: {site: (D, *site shape) tensor} as `HipEngine.sample_posterior` returns them ("ν", "ϕxy" and, where the model has them,
    "Δν", "shape_inv", "logγg", "logβg", "νω"; other keys are ignored).  A site that is the same in every draw (conditioned, or one
    of the guide's Delta sites) may be given with a leading dimension of 1: it then costs nothing per draw, and when everything the
    spliced term depends on is such a site, the S matrix is evaluated once (its p_waic is exactly 0).  Draws given with the full leading
    dimension are checked for that on the device.
    chunk_cells: cells per library call (rounded up to a multiple of 64; default: all).  The result does not depend on it.
    Results are for this engine's cells, in the caller's order."""
    sp = engine.spec
    vel = sp.kind == "velocity"
    mats = ["S", "U"] if vel else ["S"]
    D = _draw_count(draws)
    Ng, Nc = sp.Ng, engine.Nc_local
    check_request(sp.noisemodel, D, Ng, Nc, len(mats), return_pointwise)
    if engine.stats["generic"]:
        raise NotImplementedError(f"pointwise_density: this engine runs the run-time-sized kernel set (H = {sp.H}, Hw = {sp.Hw}, Nb = {sp.Nb}): "
                                  "only what the compiled fast set covers is supported")
    dev = engine.device
    nb = sp.noisemodel == "NegativeBinomial"
    need = {"ϕxy": (Nc, 2), "ν": (Ng, sp.Nh)}
    if sp.with_delta_nu and sp.Nb > 0:
        need["Δν"] = (sp.Nb, Ng)
    if nb:
        need["shape_inv"] = (Ng,)
    if vel:
        need.update({"logγg": (Ng,), "logβg": (Ng,), "νω": (sp.Nx, sp.Nhw)})
    fixed_sites = {"Δν", "shape_inv"}                     # Delta sites of both guides: one value
    ptr, stride, keep = {}, {}, []
    for name, shape in need.items():
        if name not in draws:
            raise ValueError(f"draws lacks the site {name!r} of this model")
        t = torch.as_tensor(draws[name]).to(device=dev, dtype=torch.float32)
        n = int(math.prod(shape))
        if t.numel() == n:
            t = t.reshape(1, n)
        elif t.numel() == D * n and t.shape[0] == D:
            t = t.reshape(D, n)
        else:
            raise ValueError(f"draws[{name!r}] has shape {tuple(t.shape)}, expected ({D} or 1, {', '.join(map(str, shape))})")
        if t.shape[0] > 1:
            same = bool((t == t[:1]).all())               # one device comparison per full-length site
            if not same and (name in fixed_sites or name in sp.condition_on):
                raise ValueError(f"draws[{name!r}] differs between draws, but the site is {'conditioned' if name in sp.condition_on else 'a Delta site'}")
            if same:
                t = t[:1]
        t = t.contiguous()
        keep.append(t)
        ptr[name] = C.c_void_p(t.data_ptr())
        stride[name] = 0 if t.shape[0] == 1 else n
    nq = 3 * len(mats)
    gene = torch.zeros((nq, Ng), dtype=torch.float64, device=dev)
    cell = torch.zeros((nq, Nc), dtype=torch.float64, device=dev)
    dense = torch.empty((len(mats), Ng, Nc), dtype=torch.float32, device=dev) if return_pointwise else None
    step = Nc if not chunk_cells else max(CELL_ALIGN, -(-int(chunk_cells) // CELL_ALIGN) * CELL_ALIGN)
    g = lambda k: ptr.get(k)
    for c0 in range(0, Nc, step):
        engine._check(engine.lib.vc_pointwise_density(
            engine._h, C.c_int64(D), g("ϕxy"), C.c_int64(stride["ϕxy"]), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"),
            g("logγg"), C.c_int64(stride.get("logγg", 0)), g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"),
            C.c_int64(stride.get("νω", 0)), C.c_int64(c0), C.c_int64(min(step, Nc - c0)), C.c_void_p(gene.data_ptr()),
            C.c_void_p(cell.data_ptr()), C.c_void_p(dense.data_ptr()) if dense is not None else None, engine._stream()))
    torch.cuda.synchronize(dev)
    del keep
    gene, cell = gene.cpu(), cell.cpu()
    pick = lambda src, j: {m: src[3 * i + j].clone() for i, m in enumerate(mats)}
    return PredictiveDensity(lppd_gene=pick(gene, 0), lppd_cell=pick(cell, 0), mean_gene=pick(gene, 1), mean_cell=pick(cell, 1),
                             p_waic_gene=pick(gene, 2), p_waic_cell=pick(cell, 2), n_draws=D,
                             pointwise=None if dense is None else {m: dense[i].cpu() for i, m in enumerate(mats)})


def merge_shards(parts) -> PredictiveDensity:
    """The records of the ranks of a cell-sharded evaluation, in rank order, as one record: per-cell results concatenated, per-gene
    results added in rank order in float64."""
    parts = list(parts)
    first = parts[0]
    cat = lambda f: {m: torch.cat([getattr(p, f)[m] for p in parts]) for m in getattr(first, f)}

    def add(f):
        out = {}
        for m in getattr(first, f):
            acc = getattr(first, f)[m].clone()
            for p in parts[1:]:
                acc = acc + getattr(p, f)[m]
            out[m] = acc
        return out
    pw = None
    if first.pointwise is not None:
        pw = {m: torch.cat([p.pointwise[m] for p in parts], dim=1) for m in first.pointwise}
    return PredictiveDensity(lppd_gene=add("lppd_gene"), lppd_cell=cat("lppd_cell"), mean_gene=add("mean_gene"), mean_cell=cat("mean_cell"),
                             p_waic_gene=add("p_waic_gene"), p_waic_cell=cat("p_waic_cell"), n_draws=first.n_draws, pointwise=pw)


def compare(a: PredictiveDensity, b: PredictiveDensity):
    """Paired difference of two fits of the same cells: (elpd_diff, standard error).  elpd_diff = sum_c (a - b) of elpd_waic per cell
    (count matrices added), se = sqrt(Nc var_c(diff_c)); positive: the data support `a`."""
    da = sum(a.elpd_waic_cell.values())
    db = sum(b.elpd_waic_cell.values())
    if da.shape != db.shape:
        raise ValueError(f"compare: the records hold {da.numel()} and {db.numel()} cells; only fits of the same cells can be compared")
    diff = (da - db).double()
    n = diff.numel()
    se = math.sqrt(n * float(diff.var(unbiased=True))) if n > 1 else float("nan")
    return float(diff.sum()), se
