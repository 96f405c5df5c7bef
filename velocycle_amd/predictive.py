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


def _check_noisemodel(fn: str, noisemodel: str):
    """The noise models the draw kernels (csrc/vc_draw_model.h) cover, for pointwise_density and predictive_check (`fn`)."""
    if noisemodel == "Lognormal":
        raise NotImplementedError(f"{fn}: Lognormal noise is not supported (NegativeBinomial or Poisson)")
    if noisemodel not in ("NegativeBinomial", "Poisson"):
        raise ValueError(f"{noisemodel} not allowed")


def _check_fast_set(fn: str, engine):
    sp = engine.spec
    if engine.stats["generic"]:
        raise NotImplementedError(f"{fn}: this engine runs the run-time-sized kernel set (H = {sp.H}, Hw = {sp.Hw}, Nb = {sp.Nb}): "
                                  "only what the compiled fast set covers is supported")


def check_request(noisemodel: str, n_draws: int, Ng: int, Nc: int, n_matrices: int, return_pointwise: bool):
    """The refusals that need no device: raised before any library or GPU call."""
    _check_noisemodel("pointwise_density", noisemodel)
    if int(n_draws) < 2:
        raise ValueError(f"pointwise_density needs at least 2 draws (the variance over draws divides by n - 1), got {n_draws}")
    if return_pointwise and 4 * int(Ng) * int(Nc) * int(n_matrices) > MAX_POINTWISE_BYTES:
        raise ValueError(f"return_pointwise: the dense lppd of {n_matrices} x {Ng} x {Nc} elements exceeds {MAX_POINTWISE_BYTES} bytes; "
                         "use the per-gene / per-cell sums")


def _draw_count(draws, phixy: bool = True) -> int:
    """phixy=False (phase_marginal): 'ϕxy' is neither required nor counted."""
    if "ν" not in draws or (phixy and "ϕxy" not in draws):
        raise ValueError("draws must hold at least the sites 'ν' and 'ϕxy' (what HipEngine.sample_posterior returns)" if phixy else
                         "draws must hold at least the site 'ν'")
    # a site that is the same in every draw may be given once: the number of draws is the longest leading dimension
    return max(int(draws[k].shape[0]) for k in ("ν", "ϕxy", "logγg", "logβg", "νω") if k in draws and (phixy or k != "ϕxy"))


def _device_draws(engine, draws, D, phixy: bool = True):
    """The sites of this engine's model out of `draws` as contiguous float32 device tensors: ({site: pointer}, {site: draw stride in
    floats, 0 for a site that is the same in every draw}, the tensors to keep alive).  phixy=False: without 'ϕxy'."""
    sp = engine.spec
    vel = sp.kind == "velocity"
    Ng, Nc = sp.Ng, engine.Nc_local
    dev = engine.device
    nb = sp.noisemodel == "NegativeBinomial"
    need = {"ϕxy": (Nc, 2), "ν": (Ng, sp.Nh)}
    if sp.with_delta_nu and sp.Nb > 0:
        need["Δν"] = (sp.Nb, Ng)
    if nb:
        need["shape_inv"] = (Ng,)
    if vel:
        need.update({"logγg": (Ng,), "logβg": (Ng,), "νω": (sp.Nx, sp.Nhw)})
    if not phixy:
        del need["ϕxy"]
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
    return ptr, stride, keep


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
    _check_fast_set("pointwise_density", engine)
    dev = engine.device
    ptr, stride, keep = _device_draws(engine, draws, D)
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


# ----------------------------------------------------------------------------------------------------------------------------------
# posterior predictive check: replicated counts over posterior draws (vc_predictive_check, csrc/vc_ppc.hip), the device count
# sampler on its own (vc_sample_counts, csrc/vc_count_sampler.h)
# ----------------------------------------------------------------------------------------------------------------------------------
STATISTICS = ("mean", "variance", "zero_fraction", "max")
SAMPLER_MU_MAX = float(1 << 20)      # supported range of the sampler's Poisson rate (VC_CS_MU_MAX)


def _p_values(rep, obs, n):
    ge = (rep >= obs).sum(0).double() / n
    gt = (rep > obs).sum(0).double() / n
    return {"p_ge": ge, "p_gt": gt, "p_mid": 0.5 * (ge + gt)}


@dataclass
class PredictiveCheck:
    """Replicated-count statistics of a fit, per count matrix {"S": ..., "U": ...}, CPU tensors.

    gene_rep[m]  (D, 4, Ng) int64: per draw and gene, over the record's cells: sum k, sum k^2, #{k = 0}, max k of the replicates
    cell_rep[m]  (D, Nc) int64: per draw and cell, sum k over the genes (the replicated library size)
    gene_obs[m]  (4, Ng) float64, cell_obs[m] (Nc,) float64: the same statistics of the observed counts
    replicates[m] (n_keep, Ng, Nc) int32 of the first n_keep draws, when asked for.
    Derived (float64, formed on the host): `gene_T_rep` (D, 4, Ng) / `gene_T_obs` (4, Ng) with T in STATISTICS order (the variance is
    sum k^2 / n - mean^2), and `gene(stat)` / `library_size()`: replicate mean and sd over draws, p_ge = #{d: T_rep >= T_obs} / D,
    p_gt, p_mid = (p_ge + p_gt) / 2."""
    gene_rep: Dict[str, torch.Tensor]
    cell_rep: Dict[str, torch.Tensor]
    gene_obs: Dict[str, torch.Tensor]
    cell_obs: Dict[str, torch.Tensor]
    n_draws: int
    n_cells: int
    seed: int
    replicates: Optional[Dict[str, torch.Tensor]] = None

    @staticmethod
    def _T(tab, n):
        t = tab.double()
        mean = t[..., 0, :] / n
        return torch.stack([mean, t[..., 1, :] / n - mean * mean, t[..., 2, :] / n, t[..., 3, :]], dim=-2)

    @property
    def gene_T_rep(self):
        return {m: self._T(v, self.n_cells) for m, v in self.gene_rep.items()}

    @property
    def gene_T_obs(self):
        return {m: self._T(v, self.n_cells) for m, v in self.gene_obs.items()}

    @staticmethod
    def _summary(rep, obs, n):
        out = {"obs": obs, "rep_mean": rep.mean(0), "rep_sd": rep.std(0, unbiased=True) if n > 1 else torch.zeros_like(obs)}
        out.update(_p_values(rep, obs, n))
        return out

    def gene(self, stat: str):
        """{matrix: {"obs", "rep_mean", "rep_sd", "p_ge", "p_gt", "p_mid"}: (Ng,) float64} of one of STATISTICS."""
        j = STATISTICS.index(stat)
        rep, obs = self.gene_T_rep, self.gene_T_obs
        return {m: self._summary(rep[m][:, j], obs[m][j], self.n_draws) for m in rep}

    def library_size(self):
        """{matrix: {...}: (Nc,) float64}: the same summary of the per-cell sum over genes."""
        return {m: self._summary(self.cell_rep[m].double(), self.cell_obs[m], self.n_draws) for m in self.cell_rep}


def check_ppc_request(noisemodel: str, n_draws: int, Ng: int, Nc: int, n_matrices: int, keep_replicates: int):
    """The refusals of predictive_check that need no device: raised before any library or GPU call."""
    _check_noisemodel("predictive_check", noisemodel)
    if int(n_draws) < 1:
        raise ValueError(f"predictive_check needs at least 1 draw, got {n_draws}")
    if not 0 <= int(keep_replicates) <= int(n_draws):
        raise ValueError(f"keep_replicates must lie in [0, {n_draws}], got {keep_replicates}")
    if 4 * int(keep_replicates) * int(Ng) * int(Nc) * int(n_matrices) > MAX_POINTWISE_BYTES:
        raise ValueError(f"keep_replicates: the dense replicates of {keep_replicates} x {n_matrices} x {Ng} x {Nc} elements exceed "
                         f"{MAX_POINTWISE_BYTES} bytes; use the per-draw statistics")


def predictive_check(engine, draws: Dict[str, torch.Tensor], *, seed: int, keep_replicates: int = 0,
                     chunk_cells: Optional[int] = None, chunk_draws: Optional[int] = None) -> PredictiveCheck:
    """Replicated counts of this engine's cells under explicit draws (as `pointwise_density` takes them), reduced on the device to
    per-draw statistics; nothing of size D x Ng x Nc exists unless keep_replicates asks for the first draws' replicates.
    seed: Philox key of the count sampler; a replicate depends on (seed, draw, matrix, gene, global cell) and its latents alone.
    chunk_cells / chunk_draws: cells / draws per library call (default: all); the result does not depend on them."""
    sp = engine.spec
    vel = sp.kind == "velocity"
    mats = ["S", "U"] if vel else ["S"]
    D = _draw_count(draws)
    Ng, Nc = sp.Ng, engine.Nc_local
    n_keep = int(keep_replicates)
    check_ppc_request(sp.noisemodel, D, Ng, Nc, len(mats), n_keep)
    _check_fast_set("predictive_check", engine)
    dev = engine.device
    ptr, stride, keep = _device_draws(engine, draws, D)
    nm = len(mats)
    gene_rep = torch.zeros((D, nm, 4, Ng), dtype=torch.int64, device=dev)
    cell_rep = torch.zeros((D, nm, Nc), dtype=torch.int64, device=dev)
    gene_obs = torch.zeros((nm, 4, Ng), dtype=torch.float64, device=dev)
    cell_obs = torch.zeros((nm, Nc), dtype=torch.float64, device=dev)
    dense = torch.zeros((n_keep, nm, Ng, Nc), dtype=torch.int32, device=dev) if n_keep else None
    cstep = Nc if not chunk_cells else max(1, int(chunk_cells))
    dstep = D if not chunk_draws else max(1, int(chunk_draws))
    g = lambda k: ptr.get(k)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for c0 in range(0, Nc, cstep):
        for d0 in range(0, D, dstep):
            first = d0 == 0                               # the observed statistics of a set of cells are formed once
            engine._check(engine.lib.vc_predictive_check(
                engine._h, C.c_int64(D), g("ϕxy"), C.c_int64(stride["ϕxy"]), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"),
                g("logγg"), C.c_int64(stride.get("logγg", 0)), g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"),
                C.c_int64(stride.get("νω", 0)), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int64(c0), C.c_int64(min(cstep, Nc - c0)),
                C.c_int64(d0), C.c_int64(min(dstep, D - d0)), vp(gene_rep), vp(cell_rep), vp(gene_obs) if first else None,
                vp(cell_obs) if first else None, vp(dense), C.c_int64(n_keep), engine._stream()))
    torch.cuda.synchronize(dev)
    del keep
    pick = lambda t, ax: {m: t.select(ax, i).cpu().clone() for i, m in enumerate(mats)}
    return PredictiveCheck(gene_rep=pick(gene_rep, 1), cell_rep=pick(cell_rep, 1), gene_obs=pick(gene_obs, 0), cell_obs=pick(cell_obs, 0),
                           n_draws=D, n_cells=Nc, seed=int(seed), replicates=None if dense is None else pick(dense, 1))


def merge_check_shards(parts) -> PredictiveCheck:
    """The records of the ranks of a cell-sharded check, in rank order, as one record: per-gene sums added, the max taken as max,
    per-cell tables (and kept replicates) concatenated.  Integer tables merge exactly; the observed sums are added in rank order."""
    parts = list(parts)
    first = parts[0]
    if any(p.n_draws != first.n_draws or p.seed != first.seed for p in parts):
        raise ValueError("merge_check_shards: the records come from different draws or seeds")

    def genes(f):
        out = {}
        for m in getattr(first, f):
            acc = getattr(first, f)[m].clone()
            for p in parts[1:]:
                t = getattr(p, f)[m]
                acc[..., :3, :] = acc[..., :3, :] + t[..., :3, :]
                acc[..., 3, :] = torch.maximum(acc[..., 3, :], t[..., 3, :])
            out[m] = acc
        return out
    cat = lambda f, dim: {m: torch.cat([getattr(p, f)[m] for p in parts], dim=dim) for m in getattr(first, f)}
    reps = None if first.replicates is None else cat("replicates", 2)
    return PredictiveCheck(gene_rep=genes("gene_rep"), cell_rep=cat("cell_rep", 1), gene_obs=genes("gene_obs"), cell_obs=cat("cell_obs", 0),
                           n_draws=first.n_draws, n_cells=sum(p.n_cells for p in parts), seed=first.seed, replicates=reps)


def sample_counts(eta: torch.Tensor, shape_inv: Optional[torch.Tensor] = None, *, seed: int, draw: int = 0, matrix: int = 0,
                  index_origin: int = 0, row_index_stride: Optional[int] = None) -> torch.Tensor:
    """Counts k ~ Poisson(exp(eta)) (shape_inv None) or GammaPoisson(1 / shape_inv, 1 / (shape_inv exp(eta))) on the device: int32
    tensor of eta's shape (vc_sample_counts).  eta: float32 DEVICE tensor, natural-log means, 1-D or (rows, columns); shape_inv: one
    value per row.  Element (i, j) is a pure function of (seed, draw, matrix, index_origin + i * row_index_stride + j, eta, shape_inv);
    row_index_stride defaults to the number of columns.  Exact samplers, rates up to 2^20 (`SAMPLER_MU_MAX`): an element beyond it
    raises `CountSamplerRangeError`.  There is no CPU path."""
    from . import _lib
    if not eta.is_cuda:
        raise ValueError("sample_counts: eta must be a device tensor (there is no CPU path)")
    if eta.dim() not in (1, 2) or eta.numel() == 0:
        raise ValueError(f"sample_counts: eta must be a non-empty 1-D or 2-D tensor, got shape {tuple(eta.shape)}")
    e = eta.to(torch.float32).contiguous()
    rows, cols = (1, e.shape[0]) if e.dim() == 1 else (e.shape[0], e.shape[1])
    si = None
    if shape_inv is not None:
        si = torch.as_tensor(shape_inv, dtype=torch.float32).to(e.device).reshape(-1).contiguous()
        if si.numel() != rows:
            raise ValueError(f"sample_counts: shape_inv holds {si.numel()} values for {rows} row(s)")
    lib = _lib.load()
    out = torch.empty(e.shape, dtype=torch.int32, device=e.device)
    with torch.cuda.device(e.device):
        rc = lib.vc_sample_counts(C.c_void_p(e.data_ptr()), C.c_int64(rows), C.c_int64(cols), C.c_void_p(si.data_ptr()) if si is not None else None,
                                  C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int64(int(draw)), C.c_int(int(matrix)), C.c_int64(int(index_origin)),
                                  C.c_int64(cols if row_index_stride is None else int(row_index_stride)), C.c_void_p(out.data_ptr()),
                                  C.c_void_p(torch.cuda.current_stream(e.device).cuda_stream))
    if rc != _lib.VC_OK:
        msg = lib.vc_last_error(None).decode()
        if rc == _lib.VC_ERR_RANGE:
            raise _lib.CountSamplerRangeError(msg)
        raise (ValueError if rc == _lib.VC_ERR_ARG else RuntimeError)(msg)
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# predictive PIT: randomized quantile residuals of every observed count over posterior draws (vc_predictive_pit, csrc/vc_pit.hip)
# ----------------------------------------------------------------------------------------------------------------------------------
PIT_MIN_BINS, PIT_MAX_BINS = 2, 64


def _uniformity(hist):
    """Float64 summaries of integer histograms (..., B) against the uniform distribution: Pearson's chi-square with the expected count
    n / B per bin (n: the row's total), its z-score (chi2 - (B - 1)) / sqrt(2 (B - 1)) and the share of the two edge bins (2 / B when
    uniform).  A row without elements gives NaN."""
    h = hist.double()
    B = h.shape[-1]
    n = h.sum(-1)
    expected = (n / B).unsqueeze(-1)
    chi2 = (((h - expected) ** 2) / expected).sum(-1)
    return {"chi2": chi2, "z": (chi2 - (B - 1)) / math.sqrt(2.0 * (B - 1)), "edge_share": (h[..., 0] + h[..., -1]) / n}


@dataclass
class PredictivePIT:
    """Randomized PIT values u of every observed count under the posterior predictive distribution, binned, per count matrix
    {"S": ..., "U": ...}, CPU tensors.  Calibrated: u uniform; U-shaped histograms: the model is under-dispersed; hump-shaped:
    over-dispersed; skewed: biased.

    gene_hist[m]  (Ng, bins) int64: per gene, the bins of u over the record's cells
    cell_hist[m]  (Nc, bins) int64: per cell, the bins of u over the genes
    pointwise[m]  (3, Ng, Nc) float32: F_lo = P(K <= k - 1), F_hi = P(K <= k) and u = F_lo + v (F_hi - F_lo) per element, when asked for
    Derived on the host in float64: `gene()`, `cell()`, `pooled()` -- chi-square against uniform, its z-score and the edge-bin share."""
    gene_hist: Dict[str, torch.Tensor]
    cell_hist: Dict[str, torch.Tensor]
    n_draws: int
    bins: int
    seed: int
    pointwise: Optional[Dict[str, torch.Tensor]] = None

    def gene(self):
        """{matrix: {"chi2", "z", "edge_share": (Ng,) float64}}."""
        return {m: _uniformity(h) for m, h in self.gene_hist.items()}

    def cell(self):
        """{matrix: {"chi2", "z", "edge_share": (Nc,) float64}}."""
        return {m: _uniformity(h) for m, h in self.cell_hist.items()}

    def pooled(self):
        """{matrix: {"hist": (bins,) int64, "chi2", "z", "edge_share": float}} over all elements of the matrix."""
        out = {}
        for m, h in self.gene_hist.items():
            tot = h.sum(0)
            out[m] = {"hist": tot, **{k: float(v) for k, v in _uniformity(tot).items()}}
        return out


def check_pit_request(noisemodel: str, n_draws: int, bins: int, Ng: int, Nc: int, n_matrices: int, return_pointwise: bool):
    """The refusals of predictive_pit that need no device: raised before any library or GPU call."""
    _check_noisemodel("predictive_pit", noisemodel)
    if int(n_draws) < 1:
        raise ValueError(f"predictive_pit needs at least 1 draw, got {n_draws}")
    if not PIT_MIN_BINS <= int(bins) <= PIT_MAX_BINS:
        raise ValueError(f"predictive_pit: bins must lie in [{PIT_MIN_BINS}, {PIT_MAX_BINS}], got {bins}")
    if return_pointwise and 12 * int(Ng) * int(Nc) * int(n_matrices) > MAX_POINTWISE_BYTES:
        raise ValueError(f"return_pointwise: F_lo, F_hi and u of {n_matrices} x {Ng} x {Nc} elements exceed {MAX_POINTWISE_BYTES} bytes; "
                         "use the per-gene / per-cell histograms")


def predictive_pit(engine, draws: Dict[str, torch.Tensor], *, seed: int, bins: int = 20, return_pointwise: bool = False,
                   chunk_cells: Optional[int] = None) -> PredictivePIT:
    """The randomized PIT of every observed count of this engine's cells under explicit draws (as `pointwise_density` takes them):
    histograms of u per gene and per cell, and on request F_lo, F_hi and u per element.  Nothing of size D x Ng x Nc exists.
    seed: Philox key of the randomization; u depends on (seed, matrix, gene, global cell) and the draws alone.
    chunk_cells: cells per library call (default: all); the result does not depend on it.  There is no CPU path."""
    sp = engine.spec
    vel = sp.kind == "velocity"
    mats = ["S", "U"] if vel else ["S"]
    D = _draw_count(draws)
    Ng, Nc = sp.Ng, engine.Nc_local
    B = int(bins)
    check_pit_request(sp.noisemodel, D, B, Ng, Nc, len(mats), return_pointwise)
    _check_fast_set("predictive_pit", engine)
    dev = engine.device
    ptr, stride, keep = _device_draws(engine, draws, D)
    nm = len(mats)
    gene = torch.zeros((nm, Ng, B), dtype=torch.int64, device=dev)
    cell = torch.zeros((nm, Nc, B), dtype=torch.int64, device=dev)
    dense = torch.empty((nm, 3, Ng, Nc), dtype=torch.float32, device=dev) if return_pointwise else None
    step = Nc if not chunk_cells else max(1, int(chunk_cells))
    g = lambda k: ptr.get(k)
    for c0 in range(0, Nc, step):
        engine._check(engine.lib.vc_predictive_pit(
            engine._h, C.c_int64(D), g("ϕxy"), C.c_int64(stride["ϕxy"]), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"),
            g("logγg"), C.c_int64(stride.get("logγg", 0)), g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"),
            C.c_int64(stride.get("νω", 0)), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int32(B), C.c_int64(c0),
            C.c_int64(min(step, Nc - c0)), C.c_void_p(gene.data_ptr()), C.c_void_p(cell.data_ptr()),
            C.c_void_p(dense.data_ptr()) if dense is not None else None, engine._stream()))
    torch.cuda.synchronize(dev)
    del keep
    pick = lambda t: {m: t[i].cpu().clone() for i, m in enumerate(mats)}
    return PredictivePIT(gene_hist=pick(gene), cell_hist=pick(cell), n_draws=D, bins=B, seed=int(seed),
                         pointwise=None if dense is None else pick(dense))


def merge_pit_shards(parts) -> PredictivePIT:
    """The records of the ranks of a cell-sharded evaluation, in rank order, as one record: the per-gene histograms added (integers:
    exact), the per-cell histograms and the dense columns concatenated."""
    parts = list(parts)
    first = parts[0]
    if any(p.n_draws != first.n_draws or p.seed != first.seed or p.bins != first.bins for p in parts):
        raise ValueError("merge_pit_shards: the records come from different draws, seeds or bins")
    if any((p.pointwise is None) != (first.pointwise is None) for p in parts):
        raise ValueError("merge_pit_shards: only some of the records hold pointwise values")
    gene = {m: torch.stack([p.gene_hist[m] for p in parts]).sum(0) for m in first.gene_hist}
    cell = {m: torch.cat([p.cell_hist[m] for p in parts], dim=0) for m in first.cell_hist}
    pw = None if first.pointwise is None else {m: torch.cat([p.pointwise[m] for p in parts], dim=2) for m in first.pointwise}
    return PredictivePIT(gene_hist=gene, cell_hist=cell, n_draws=first.n_draws, bins=first.bins, seed=first.seed, pointwise=pw)


# ----------------------------------------------------------------------------------------------------------------------------------
# phase-marginal scoring: the phase posterior of every cell on a grid and its evidence with the phase integrated out
# (vc_phase_marginal, csrc/vc_phase_marginal.hip)
# ----------------------------------------------------------------------------------------------------------------------------------
PM_MIN_BINS, PM_MAX_BINS = 2, 4096
PHASE_PRIORS = ("model", "flat")
_PN_ASYMPTOTIC = 12.0                # beyond this |t| the cancelling 1 - s R(s) of the projected normal is summed as a series


def projected_normal_logpdf(m: torch.Tensor, phi: torch.Tensor) -> torch.Tensor:
    """log density of the angle of x ~ Normal(m, I) in the plane (the projected normal), float64:
    p(phi) = (1 / 2 pi) exp(-|m|^2 / 2) [1 + t Phi(t) / phi(t)],  t = m . (cos phi, sin phi).
    m: (..., 2), phi broadcastable against m[..., 0].  t >= 0: log1p of exp(log t + log_ndtr(t) + t^2 / 2 + log sqrt(2 pi)); t < 0:
    1 - s R(s), s = -t, R the Mills ratio, which cancels: directly up to s = 12 (error ~ s^4 eps), beyond by its asymptotic series
    sum_n (-1)^(n+1) (2n - 1)!! / s^(2n)."""
    m = torch.as_tensor(m, dtype=torch.float64)
    phi = torch.as_tensor(phi, dtype=torch.float64)
    t = m[..., 0] * torch.cos(phi) + m[..., 1] * torch.sin(phi)
    half_log_2pi = 0.5 * math.log(2.0 * math.pi)
    tp = t.clamp(min=1e-300)
    pos = torch.nn.functional.softplus(torch.log(tp) + torch.special.log_ndtr(tp) + 0.5 * tp * tp + half_log_2pi, threshold=700.0)
    s = (-t).clamp(min=0.0)
    sm = s.clamp(max=_PN_ASYMPTOTIC)
    direct = torch.log1p(-sm * torch.exp(torch.special.log_ndtr(-sm) + 0.5 * sm * sm + half_log_2pi))
    sl = s.clamp(min=_PN_ASYMPTOTIC)
    inv2 = 1.0 / (sl * sl)
    term = inv2.clone()
    series = term.clone()
    for n in range(2, 21):
        term = -term * (2 * n - 1) * inv2
        series = series + term
    neg = torch.where(s > _PN_ASYMPTOTIC, torch.log(series), direct)
    bracket = torch.where(t > 0, pos, neg)
    return -math.log(2.0 * math.pi) - 0.5 * (m * m).sum(-1) + bracket


def phase_grid(bins: int) -> torch.Tensor:
    """phi_j = 2 pi j / bins, float64 (the grid of the reference's from_cycle_mle, phases.py:495)."""
    return 2.0 * math.pi * torch.arange(int(bins), dtype=torch.float64) / int(bins)


def phase_log_prior(phixy_prior: torch.Tensor, bins: int) -> torch.Tensor:
    """(Nc, bins) float64 log prior mass of every grid bin under the model's Normal(ϕxy_prior[c], I) on the direction
    (velocity_inference_model.py:337): the projected-normal density at the grid phases, normalised to mass 1 on the grid."""
    m = torch.as_tensor(phixy_prior, dtype=torch.float64).reshape(-1, 2)
    lp = projected_normal_logpdf(m[:, None, :], phase_grid(bins)[None, :])
    return lp - torch.logsumexp(lp, dim=1, keepdim=True)


def projected_normal_resultant(kappa) -> torch.Tensor:
    """Mean resultant length of the projected normal of Normal(m, I), |m| = kappa: sqrt(pi / 8) kappa e^(-z) (I0(z) + I1(z)), z = kappa^2 / 4."""
    k = torch.as_tensor(kappa, dtype=torch.float64)
    z = 0.25 * k * k
    return math.sqrt(math.pi / 8.0) * k * (torch.special.i0e(z) + torch.special.i1e(z))


def concentration_of_resultant(R, kappa_max: float = 1.0e3) -> torch.Tensor:
    """The kappa in [0, kappa_max] whose projected normal has mean resultant length R (monotone: bisection in float64)."""
    R = torch.as_tensor(R, dtype=torch.float64).clamp(0.0, 1.0)
    lo, hi = torch.zeros_like(R), torch.full_like(R, float(kappa_max))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        below = projected_normal_resultant(mid) < R
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    return 0.5 * (lo + hi)


@dataclass
class PhaseMarginal:
    """The phase of every cell integrated over a grid, CPU tensors.

    log_evidence (Nc,) float64: log (1/D) sum_d sum_j exp a[d,c,j], the cell's log predictive density with the phase integrated out
    posterior    (Nc, bins) float32: the phase posterior on the grid; rows sum to 1
    phis         (bins,) float64: the grid 2 pi j / bins
    per_draw     (D, Nc) float64 log sum_j exp a[d,c,j], when asked for."""
    log_evidence: torch.Tensor
    posterior: torch.Tensor
    phis: torch.Tensor
    n_draws: int
    per_draw: Optional[torch.Tensor] = None

    def _moments(self):
        p = self.posterior.double()
        return p @ torch.cos(self.phis), p @ torch.sin(self.phis)

    @property
    def mean_phase(self) -> torch.Tensor:
        """Circular mean of the posterior in [0, 2 pi), (Nc,) float64."""
        c, s = self._moments()
        return torch.remainder(torch.atan2(s, c), 2.0 * math.pi)

    @property
    def resultant_length(self) -> torch.Tensor:
        c, s = self._moments()
        return torch.sqrt(c * c + s * s)

    @property
    def entropy(self) -> torch.Tensor:
        """-sum_j post log post of every row (0 log 0 = 0); log(bins) for a flat row."""
        p = self.posterior.double()
        return -(torch.where(p > 0, p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p))).sum(1)

    @property
    def map_phase(self) -> torch.Tensor:
        return self.phis[self.posterior.argmax(1)]

    @property
    def elpd(self) -> float:
        return float(self.log_evidence.sum())


def check_marginal_request(noisemodel: str, n_draws: int, bins: int, Nc: int, phase_prior):
    """The refusals of phase_marginal that need no device: raised before any library or GPU call."""
    _check_noisemodel("phase_marginal", noisemodel)
    if int(n_draws) < 1:
        raise ValueError(f"phase_marginal needs at least 1 draw, got {n_draws}")
    if int(bins) != bins or not PM_MIN_BINS <= int(bins) <= PM_MAX_BINS:
        raise ValueError(f"phase_marginal: bins must be an integer in [{PM_MIN_BINS}, {PM_MAX_BINS}], got {bins}")
    if isinstance(phase_prior, str):
        if phase_prior not in PHASE_PRIORS:
            raise ValueError(f"phase_marginal: phase_prior must be one of {PHASE_PRIORS} or a (cells, bins) tensor of log masses, got {phase_prior!r}")
    elif tuple(torch.as_tensor(phase_prior).shape) != (int(Nc), int(bins)):
        raise ValueError(f"phase_marginal: the prior tensor has shape {tuple(torch.as_tensor(phase_prior).shape)}, expected ({Nc}, {bins})")


def phase_marginal(engine, draws: Dict[str, torch.Tensor], *, bins: int = 128, phase_prior="model", return_per_draw: bool = False,
                   chunk_cells: Optional[int] = None) -> PhaseMarginal:
    """The phase posterior on a grid of `bins` phases and the evidence with the phase integrated out, of every cell this engine holds,
    under explicit draws of the gene-level and global sites (as `pointwise_density` takes them; "ϕxy" is ignored and not required).
    The engine's cells need not be cells a fit has seen: a held-out cell's predictive density is this evidence.
    phase_prior: "flat" (log mass -log bins), "model" (the angle density of the model's Normal(ϕxy_prior[c], I), `phase_log_prior`,
    formed on the host in float64) or a (cells, bins) tensor of log masses, used as given (the device reads float32).
    chunk_cells: cells per library call (default: all); the result does not depend on it.  For the velocity model the integrand is not
    smooth in the phase: the evidence is that of the discrete grid.  There is no CPU path."""
    sp = engine.spec
    D = _draw_count(draws, phixy=False)
    Ng, Nc = sp.Ng, engine.Nc_local
    check_marginal_request(sp.noisemodel, D, bins, Nc, phase_prior)
    _check_fast_set("phase_marginal", engine)
    B = int(bins)
    dev = engine.device
    if isinstance(phase_prior, str):
        lw = None if phase_prior == "flat" else phase_log_prior(torch.as_tensor(sp.phixy_prior)[engine.c0:engine.c1], B)
    else:
        lw = torch.as_tensor(phase_prior)
    if lw is not None:
        lw = lw.to(device=dev, dtype=torch.float32).contiguous()
    ptr, stride, keep = _device_draws(engine, draws, D, phixy=False)
    evidence = torch.empty((Nc,), dtype=torch.float64, device=dev)
    post = torch.empty((Nc, B), dtype=torch.float32, device=dev)
    per_draw = torch.empty((D, Nc), dtype=torch.float64, device=dev) if return_per_draw else None
    step = Nc if not chunk_cells else max(1, int(chunk_cells))
    g = lambda k: ptr.get(k)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for c0 in range(0, Nc, step):
        engine._check(engine.lib.vc_phase_marginal(
            engine._h, C.c_int64(D), g("ν"), C.c_int64(stride["ν"]), g("Δν"), g("shape_inv"), g("logγg"), C.c_int64(stride.get("logγg", 0)),
            g("logβg"), C.c_int64(stride.get("logβg", 0)), g("νω"), C.c_int64(stride.get("νω", 0)), C.c_int32(B), vp(lw), C.c_int64(c0),
            C.c_int64(min(step, Nc - c0)), vp(evidence), vp(post), vp(per_draw), engine._stream()))
    torch.cuda.synchronize(dev)
    del keep
    return PhaseMarginal(log_evidence=evidence.cpu(), posterior=post.cpu(), phis=phase_grid(B), n_draws=D,
                         per_draw=None if per_draw is None else per_draw.cpu())


def merge_marginal_shards(parts) -> PhaseMarginal:
    """The records of the ranks of a cell-sharded evaluation, in rank order, as one record: every table concatenated over the cells."""
    parts = list(parts)
    first = parts[0]
    if any(p.n_draws != first.n_draws or p.posterior.shape[1] != first.posterior.shape[1] for p in parts):
        raise ValueError("merge_marginal_shards: the records come from different draws or grids")
    if any((p.per_draw is None) != (first.per_draw is None) for p in parts):
        raise ValueError("merge_marginal_shards: only some of the records hold per-draw values")
    return PhaseMarginal(log_evidence=torch.cat([p.log_evidence for p in parts]), posterior=torch.cat([p.posterior for p in parts], dim=0),
                         phis=first.phis, n_draws=first.n_draws,
                         per_draw=None if first.per_draw is None else torch.cat([p.per_draw for p in parts], dim=1))


def compare_evidence(a: PhaseMarginal, b: PhaseMarginal):
    """Paired difference of two scorings of the same cells: (sum_c (a - b) of log_evidence, standard error sqrt(Nc var_c(diff_c)));
    positive: the cells support `a`.  Like `compare`."""
    if a.log_evidence.shape != b.log_evidence.shape:
        raise ValueError(f"compare_evidence: the records hold {a.log_evidence.numel()} and {b.log_evidence.numel()} cells; only scorings "
                         "of the same cells can be compared")
    diff = (a.log_evidence - b.log_evidence).double()
    n = diff.numel()
    se = math.sqrt(n * float(diff.var(unbiased=True))) if n > 1 else float("nan")
    return float(diff.sum()), se
