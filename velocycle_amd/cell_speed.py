"""Local velocity: the angular speed of single cells and of groups of cells, on the HIP kernel `vc_cell_speed`.

`gene_kinetics.velocity_map` fits a parametric speed (at most three coefficients shared by all cells).  Here the direction is the other
one, as `phase_mle` is to `gene_harmonics`: with the cycle ν, the phases ϕ and the kinetics (log γ, log β) of every gene fixed, the
speed of a cell is a one-parameter problem over that cell's unspliced counts,

    etaS = nu_g . zeta(phi_c) + a log n_c,   d = nu_g . d zeta / d phi (phi_c),   z = omega_c d + gamma_g
    mu_U = exp(etaS) (relu(z) + 1e-5) / beta_g,   U ~ Poisson(mu_U) | NegativeBinomial(mu_U, r),   omega_c ~ Normal(m_c, s_c) (optional)

which the kernel solves for every cell by a Newton iteration inside one launch (`cell_angular_speed`).  The sums of a pass (objective,
score, Fisher and observed information) add over cells, so any group of cells -- a phase bin, a phase bin within a condition, a
cluster -- is the same one-parameter problem over its cells: `grouped_angular_speed` runs the same rules on the host over evaluate-only
passes of the kernel.  That gives a non-parametric omega(phi) with pointwise standard errors to lay over `velocity_map`'s curve, and
`CellSpeedFit.score_z`, the score of every cell against a parametric fit, from which outlier cells are read.

Limits.  gamma, beta, nu and phi are conditioned on: every standard error here is conditional on them.  A single cell with few genes is
very noisy; groups are the intended use.  The relu kink of the model is neither smoothed nor reparametrised (`n_clamped` counts the
genes at z <= 0).  Three harmonics (K = 7), Lognormal noise and batch offsets of the cycle (Δν) are refused.  The statistic
sum_c score_c^2 / fisher_c at a common start has no p-value here: its null distribution under estimated gamma, beta is not established.

Cells are independent: they are staged in chunks exactly as `phase_mle` stages them (a cell needs all of its genes), and the result does
not depend on the chunk size, the storage or the layer's format bit for bit.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .gene_harmonics import _check_cells, _dispersion_to_r, _open_device, _ptr, _row_sums, fourier_basis_from_directions
from .phase_mle import NOISEMODELS, _dense_block, _is_sparse, default_chunk_cells, u16_bits

EPS32 = float(np.finfo(np.float32).eps)
BOUND = 30.0                         # csrc/vc_cell_speed.hip
MAX_HALVINGS = 30
GROUP_PRIOR = (0.0, 3.0)             # AngularSpeed.trivial_prior's constant: mean, sd
STATUS = {_lib.VC_CSP_CONVERGED: "CONVERGED", _lib.VC_CSP_ROUNDING: "ROUNDING", _lib.VC_CSP_MAX_ITER: "MAX_ITER",
          _lib.VC_CSP_UNBOUNDED: "UNBOUNDED", _lib.VC_CSP_NO_DATA: "NO_DATA", _lib.VC_CSP_EVALUATED: "EVALUATED"}
SUMS = ("L", "score", "fisher", "observed", "N", "A")     # the columns of the kernel's sums_dev


@dataclass
class CellSpeedFit:
    """Host arrays [Nc], float64 unless said.  omega: the cell's angular speed at the last accepted point; stds = (fisher + 1 / s^2)^-1/2
    there (the Fisher standard error, conditional on nu, phi, gamma, beta); var: the inverse of the matrix the last decrement was formed
    with (observed + 1 / s^2 where positive, else Fisher); loglik: the full log-likelihood of the cell's unspliced counts (without the
    prior); score (without the prior term), fisher, observed; dec; rounding = N and magnitude = A, the scales of the kernel's rounding
    rule and of its halving allowance; iterations, status, n_clamped: int32 (`STATUS` names the codes; n_clamped = genes with z <= 0).
    score_z = score / sqrt(fisher) AT THE START: with `start` a parametric fit's speed it is each cell's score against that fit,
    approximately standard normal for a cell the fit describes."""
    omega: np.ndarray
    stds: np.ndarray
    var: np.ndarray
    loglik: np.ndarray
    score: np.ndarray
    fisher: np.ndarray
    observed: np.ndarray
    dec: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    n_clamped: np.ndarray
    score_z: np.ndarray
    rounding: np.ndarray
    magnitude: np.ndarray


@dataclass
class GroupSpeedFit:
    """Host arrays [G], float64 unless said.  omega, stds (Fisher, with the prior's precision), var (of the last decrement's matrix),
    loglik (full, of the group's cells, without the prior), score, fisher, observed, dec; rounds: steps taken, status (`STATUS`),
    n_cells (cells with a count), n_clamped ((cell, gene) pairs with z <= 0): int32.  An empty group is NO_DATA with NaN."""
    omega: np.ndarray
    stds: np.ndarray
    var: np.ndarray
    loglik: np.ndarray
    score: np.ndarray
    fisher: np.ndarray
    observed: np.ndarray
    dec: np.ndarray
    rounds: np.ndarray
    status: np.ndarray
    n_cells: np.ndarray
    n_clamped: np.ndarray


def _per_item(value, n, what, unit):
    v = np.asarray(value, dtype=np.float64).reshape(-1)
    if v.size == 1:
        v = np.broadcast_to(v, (n,)).copy()
    if v.size != n:
        raise ValueError(f"{what} must be a scalar or one value per {unit} ({n}), got {v.size}")
    return np.ascontiguousarray(v)


def _check_prior(prior, n, unit):
    """(mean, sd), each a scalar or one value per cell / group, or an array [n, 2] -> float64 [n, 2]; None -> None."""
    if prior is None:
        return None
    p = np.asarray(prior, dtype=np.float64) if not isinstance(prior, (tuple, list)) else None
    if p is not None and p.shape == (n, 2):
        return np.ascontiguousarray(p)
    if len(prior) != 2:
        raise ValueError(f"the prior is (mean, sd) of the angular speed, scalars or one value per {unit}, or an array [{n}, 2]")
    return np.ascontiguousarray(np.stack([_per_item(prior[0], n, "the prior's mean", unit), _per_item(prior[1], n, "the prior's sd", unit)], 1))


def check_arguments(counts, directions, n_scounts, means, log_gammas, log_betas, a=1, noisemodel="Poisson", dispersion=0.3, genes=None,
                    tol=1e-10, max_iter=25):
    """Every refusal that needs no device.  Returns (keep: None or the kept genes' indices, basis float64 [K, Nc], logm float64 [Nc],
    nu float64 [n, K], xy float64 [n, 2], r float64 [n] or None) over the n kept genes."""
    if noisemodel not in NOISEMODELS:
        raise NotImplementedError("Not implemented yet, sorry")
    nu = np.asarray(means, dtype=np.float64)
    if nu.ndim != 2 or nu.shape[0] not in (3, 5):
        raise ValueError(f"means must be [2 harmonics + 1, genes] with 1 or 2 harmonics (3 are not instantiated, 0 have no velocity), "
                         f"got {nu.shape}")
    Nc, Ng, xy, n = _check_cells(counts, directions, n_scounts, tol, max_iter)
    if nu.shape[1] != Ng:
        raise ValueError(f"means has {nu.shape[1]} genes, counts {Ng}")
    lg, lb = np.asarray(log_gammas, dtype=np.float64).reshape(-1), np.asarray(log_betas, dtype=np.float64).reshape(-1)
    if lg.size != Ng or lb.size != Ng:
        raise ValueError(f"log_gammas and log_betas must hold one value per gene ({Ng}), got {lg.size} and {lb.size}")
    finite = np.isfinite(nu).all(0) & np.isfinite(lg) & np.isfinite(lb)
    if genes is None:
        mask = finite
    else:
        mask = np.asarray(genes)
        if mask.dtype != np.bool_ or mask.shape != (Ng,):
            raise ValueError(f"genes must be a boolean mask over the genes ({Ng},)")
        bad = int((mask & ~finite).sum())
        if bad:
            raise ValueError(f"{bad} of the {int(mask.sum())} kept genes have means, log_gammas or log_betas that are not finite")
    if not mask.any():
        raise ValueError("no gene is kept: every gene's coefficients are not finite, or the mask is empty")
    r = _dispersion_to_r(noisemodel, dispersion, Ng)
    keep = None if mask.all() else np.flatnonzero(mask)
    sel = slice(None) if keep is None else keep
    basis = fourier_basis_from_directions(xy, (nu.shape[0] - 1) // 2)
    logm = float(a) * torch.log(torch.as_tensor(n))
    return (keep, basis, logm, np.ascontiguousarray(nu.T[sel]), np.ascontiguousarray(np.stack([lg[sel], lb[sel]], 1)),
            r[sel].contiguous() if r is not None else None)


def _check_run_options(storage, chunk_cells):
    if storage not in ("auto", "f32", "u16"):
        raise ValueError(f"unknown storage {storage!r}")
    if chunk_cells is not None and int(chunk_cells) < 1:
        raise ValueError("chunk_cells must be >= 1")


def _keep_genes(counts, keep):
    if keep is None:
        return counts
    if _is_sparse(counts):
        return counts.tocsr()[:, keep]
    if torch.is_tensor(counts):
        return counts[:, torch.as_tensor(keep, device=counts.device)]
    return np.asarray(counts)[:, keep]


def _cell_constants(blk, r64):
    """The part of every cell's log-likelihood the kernel leaves out, float64 [n]: sum_g -lgamma(k + 1), and for the negative binomial
    lgamma(k + r) - lgamma(r) (its r log r is inside the kernel's objective).  blk: float32 [Ng][n]; the sum over the genes is
    `_row_sums`' halving, so a cell's bits do not depend on the cells that go with it."""
    out = torch.empty(blk.shape[1], dtype=torch.float64, device=blk.device)
    cols = max(1, (1 << 24) // blk.shape[0])
    for i in range(0, blk.shape[1], cols):
        k = blk[:, i:i + cols].double()
        t = -torch.lgamma(k + 1.0)
        if r64 is not None:
            t += torch.lgamma(k + r64[:, None]) - torch.lgamma(r64[:, None])
        out[i:i + cols] = _row_sums(t.T.contiguous())
    return out


class _Problem:
    """The cells staged on the device in chunks (kept for every pass of a grouped fit) and the kernel's launches over them.
    stride_pad: further columns between the gene rows of every block (gene_stride = cells of the chunk + stride_pad), holding counts of
    their own that no cell may read."""

    def __init__(self, counts, basis, logm, nu, xy, r, noisemodel, device, chunk_cells, storage, stride_pad=0):
        self.lib, self.dev, self.Error = _open_device(device)
        self.Nc, self.Ng, self.K = int(counts.shape[0]), int(nu.shape[0]), int(basis.shape[0])
        self.noise = _lib.NOISE[noisemodel]
        dev = self.dev
        if _is_sparse(counts):
            counts = counts.tocsr()
        with torch.cuda.device(dev):
            self.B = basis.to(torch.float32).to(dev).contiguous()
            self.logm = logm.to(torch.float32).to(dev).contiguous()
            self.nu = torch.as_tensor(nu).to(dev).contiguous()
            self.xy = torch.as_tensor(xy).to(dev).contiguous()
            self.r = r.to(torch.float32).to(dev).contiguous() if r is not None else None
            r64 = self.r.double() if self.r is not None else None                # the model is the one of the float32 r the kernel reads
            self.const = torch.empty(self.Nc, dtype=torch.float64, device=dev)
            self.chunks = []
            step = int(chunk_cells) if chunk_cells is not None else default_chunk_cells(self.Ng)
            for c0 in range(0, self.Nc, step):
                c1 = min(self.Nc, c0 + step)
                blk = _dense_block(counts, c0, c1, self.Ng, dev)
                lo, hi = float(blk.min()), float(blk.max())
                if not (lo >= 0.0 and np.isfinite(hi)):
                    raise ValueError("counts must be finite and >= 0")
                if storage == "u16" and hi > 65535:
                    raise ValueError("storage='u16' needs every count <= 65535")
                self.const[c0:c1] = _cell_constants(blk, r64)
                if stride_pad:
                    wide = torch.full((self.Ng, c1 - c0 + int(stride_pad)), 7.0, dtype=torch.float32, device=dev)
                    wide[:, :c1 - c0] = blk
                    blk = wide
                if storage != "f32" and hi <= 65535:
                    kblk, kind = u16_bits(blk), _lib.VC_COUNTS_U16
                else:
                    kblk, kind = blk, _lib.VC_COUNTS_F32
                self.chunks.append((c0, c1, kblk, kind, self.B[:, c0:c1].contiguous()))
                del blk

    def run(self, start, prior, tol, max_iter):
        """One launch per chunk from `start` (float64 [Nc], host or device) under `prior` (float64 [Nc, 2] or None).  Returns device
        tensors over all cells: omega, var, sums [Nc, 6], dec (float64), it, st, nc (int32)."""
        dev, Nc = self.dev, self.Nc
        with torch.cuda.device(dev):
            start_d = (start if torch.is_tensor(start) else torch.as_tensor(np.ascontiguousarray(start, dtype=np.float64))).to(dev).contiguous()
            prior_d = torch.as_tensor(prior).to(dev).contiguous() if prior is not None else None
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)         # noqa: E731
            i32 = lambda: torch.empty(Nc, dtype=torch.int32, device=dev)             # noqa: E731
            out = dict(omega=f64(Nc), var=f64(Nc), sums=f64(Nc, len(SUMS)), dec=f64(Nc), it=i32(), st=i32(), nc=i32())
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for c0, c1, kblk, kind, B in self.chunks:
                sl = lambda t: _ptr(t[c0:c1]) if t is not None else None             # noqa: E731
                rc = self.lib.vc_cell_speed(_ptr(kblk), kind, self.Ng, c1 - c0, int(kblk.shape[1]), _ptr(B), self.K, sl(self.logm),
                                            _ptr(self.nu), _ptr(self.xy), self.noise, _ptr(self.r), sl(prior_d), sl(start_d), float(tol),
                                            int(max_iter), sl(out["omega"]), sl(out["var"]), sl(out["sums"]), sl(out["dec"]),
                                            sl(out["it"]), sl(out["st"]), sl(out["nc"]), stream)
                if rc != _lib.VC_OK:
                    raise self.Error(f"vc_cell_speed failed ({rc}): {self.lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # start_d, prior_d and the slices outlive their launches
        return out

    def fit(self, out, prior, score_z):
        s = out["sums"].cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            pp = 0.0 if prior is None else 1.0 / np.asarray(prior, dtype=np.float64)[:, 1] ** 2
            stds = 1.0 / np.sqrt(s[:, 2] + pp)
        return CellSpeedFit(omega=out["omega"].cpu().numpy(), stds=stds, var=out["var"].cpu().numpy(),
                            loglik=(out["sums"][:, 0] + self.const).cpu().numpy(), score=s[:, 1].copy(), fisher=s[:, 2].copy(),
                            observed=s[:, 3].copy(), dec=out["dec"].cpu().numpy(), iterations=out["it"].cpu().numpy(),
                            status=out["st"].cpu().numpy(), n_clamped=out["nc"].cpu().numpy(), score_z=score_z, rounding=s[:, 4].copy(),
                            magnitude=s[:, 5].copy())


def _score_z(sums):
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums[:, 1] / np.sqrt(sums[:, 2])


def cell_angular_speed(counts_U, directions, n_scounts, means, log_gammas, log_betas, start, a=1, noisemodel="Poisson", dispersion=0.3, *,
                       prior=None, genes=None, evaluate_only=False, tol=1e-10, max_iter=25, device=None, chunk_cells=None, storage="auto"):
    """The angular speed of every cell on the HIP kernel `vc_cell_speed`: the maximum over omega_c of the log-likelihood of the cell's
    unspliced counts (under `prior`, if one is given) with everything else fixed.  counts_U: [Nc, Ng] like an AnnData layer (numpy,
    scipy sparse or torch); directions, n_scounts, a, dispersion, device, storage: as for `gene_kinetics`; means: [2H+1, Ng] like
    `Cycle.means`, H in {1, 2}; log_gammas, log_betas: [Ng] like `Cycle.log_gammas` / `Cycle.log_betas` (a `GeneKineticsFit`'s).
    start: a scalar or [Nc], where every cell starts -- the natural value is a parametric fit's speed, `nu_omega @ omega_design(...)`.
    prior: None, or (mean, sd) of omega_c ~ Normal, scalars or one value per cell (or an array [Nc, 2]).  genes: a boolean mask [Ng];
    the default keeps every gene whose coefficients are finite; a kept gene with a coefficient that is not finite is refused.
    evaluate_only=True makes one pass at `start`.  chunk_cells: cells per staged chunk (None: `phase_mle.default_chunk_cells`).
    A cell without an unspliced count in the kept genes, with a start that is not finite or a prior sd that is not finite and > 0 comes
    back NO_DATA with NaN.  Returns a `CellSpeedFit`; its `score_z` is taken at `start` (one further evaluate-only pass)."""
    keep, basis, logm, nu, xy, r = check_arguments(counts_U, directions, n_scounts, means, log_gammas, log_betas, a, noisemodel, dispersion,
                                                   genes, tol, max_iter)
    Nc = int(counts_U.shape[0])
    st = _per_item(start, Nc, "start", "cell")
    pr = _check_prior(prior, Nc, "cell")
    _check_run_options(storage, chunk_cells)
    prob = _Problem(_keep_genes(counts_U, keep), basis, logm, nu, xy, r, noisemodel, device, chunk_cells, storage)
    at_start = prob.run(st, pr, tol, 0)
    z = _score_z(at_start["sums"].cpu().numpy())
    return prob.fit(at_start if evaluate_only else prob.run(st, pr, tol, max_iter), pr, z)


def group_sums(sums, n_clamped, ok, groups, G):
    """The per-cell sums [Nc, 6] and clamped genes [Nc] of the cells with `ok` added per group in float64, every group in the order of its
    cells' positions (np.bincount walks its input once, front to back).  Returns (float64 [G, 6], clamped int64 [G], cells int64 [G])."""
    g = groups[ok]
    S = np.stack([np.bincount(g, weights=sums[ok, i], minlength=G) for i in range(sums.shape[1])], 1)
    return S, np.bincount(g, weights=n_clamped[ok].astype(np.float64), minlength=G).astype(np.int64), np.bincount(g, minlength=G)


def solve_groups(evaluate, start, pm, pp, tol, max_rounds):
    """`vc_cell_speed`'s rules on the host, for every group at once.  evaluate(omega [G]) -> (sums [G, 6], n_clamped [G], n_cells [G]) of
    one pass at the groups' speeds.  start, pm, pp: float64 [G] (the prior's mean and precision).  Returns dict(omega, cur (the sums
    at omega), n_clamped, n_cells, A (the last decrement's matrix), dec, rounds, status)."""
    G = len(start)
    om = np.clip(np.asarray(start, dtype=np.float64), -BOUND, BOUND)
    S, ncl, ncell = evaluate(om)
    cur, cl = S.copy(), ncl.copy()
    status = np.full(G, _lib.VC_CSP_MAX_ITER, dtype=np.int32)
    active = ncell > 0                                                               # a group without a cell has no fit
    status[~active] = _lib.VC_CSP_NO_DATA
    steps, halvings = np.zeros(G, dtype=np.int32), np.full(G, MAX_HALVINGS)
    Gc, Ac, dec, fcur, step, t, trial = (np.zeros(G) for _ in range(7))
    trial[:] = om

    def decide(g):
        u = om[g] - pm[g]
        Gc[g] = cur[g, 1] - pp[g] * u
        fcur[g] = cur[g, 0] - 0.5 * pp[g] * u * u
        A = cur[g, 3] + pp[g]
        if not (0.0 < A < 1e300):
            A = cur[g, 2] + pp[g]
        Ac[g] = A
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            step[g] = Gc[g] / A
            dec[g] = Gc[g] * step[g]
        stop = None
        if max_rounds == 0:
            stop = _lib.VC_CSP_EVALUATED
        elif not abs(dec[g]) < 1e300:
            stop = _lib.VC_CSP_MAX_ITER
        elif dec[g] <= tol:
            stop = _lib.VC_CSP_CONVERGED
        elif abs(Gc[g]) <= 4.0 * EPS32 * np.sqrt(cur[g, 4]):
            stop = _lib.VC_CSP_ROUNDING
        elif steps[g] >= max_rounds:
            stop = _lib.VC_CSP_MAX_ITER
        else:
            t[g], trial[g] = 1.0, om[g] + step[g]
            if not abs(trial[g]) <= BOUND:
                stop = _lib.VC_CSP_UNBOUNDED
        if stop is not None:
            status[g], active[g] = stop, False

    for g in np.flatnonzero(active):
        decide(g)
    while active.any():
        S, ncl, _ = evaluate(np.where(active, trial, om))
        for g in np.flatnonzero(active):
            u = trial[g] - pm[g]
            f2 = S[g, 0] - 0.5 * pp[g] * u * u
            if f2 >= fcur[g] - 8.0 * EPS32 * max(S[g, 5], cur[g, 5]):           # false for a NaN: such a step is halved
                om[g], cur[g], cl[g] = trial[g], S[g], ncl[g]
                steps[g] += 1
                decide(g)
            elif halvings[g] == 0:
                status[g], active[g] = _lib.VC_CSP_MAX_ITER, False
            else:
                halvings[g] -= 1
                t[g] *= 0.5
                trial[g] = om[g] + t[g] * step[g]
    return dict(omega=om, cur=cur, n_clamped=cl, n_cells=ncell, A=Ac, dec=dec, rounds=steps, status=status)


def _check_groups(groups, Nc):
    g = np.asarray(groups)
    if g.shape != (Nc,) or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"groups must be one integer per cell ({Nc},)")
    if g.min() < 0:
        raise ValueError("groups must be >= 0")
    return g.astype(np.int64)


def grouped_angular_speed(counts_U, directions, n_scounts, means, log_gammas, log_betas, groups, start, a=1, noisemodel="Poisson",
                          dispersion=0.3, *, n_groups=None, prior=None, genes=None, tol_outer=1e-10, max_rounds=30, device=None,
                          chunk_cells=None, storage="auto"):
    """One angular speed per group of cells: `cell_angular_speed`'s model with omega_c = omega[groups[c]], solved by the kernel's own
    rules (`solve_groups`) on the host over evaluate-only passes of `vc_cell_speed`, each at omega[groups].  groups: int [Nc] in
    0..G-1 (G = n_groups, or the largest label + 1; `phase_bin_groups` gives the usual ones); start: a scalar or [G].  The per-cell sums
    are added per group in float64 in the order of the cells' positions (`group_sums`): the result is the same for any `chunk_cells`
    and under repetition.  prior: (mean, sd) per group (scalars, [G] each, or an array [G, 2]); None: `AngularSpeed.trivial_prior`'s
    constant, Normal(0, 3).  tol_outer: the decrement to stop at; max_rounds: steps per group.  A cell without a count is left out
    (`n_cells` counts the others); a group without a cell is NO_DATA with NaN.  Returns a `GroupSpeedFit`."""
    keep, basis, logm, nu, xy, r = check_arguments(counts_U, directions, n_scounts, means, log_gammas, log_betas, a, noisemodel, dispersion,
                                                   genes, tol_outer, 1)
    Nc = int(counts_U.shape[0])
    grp = _check_groups(groups, Nc)
    G = int(grp.max()) + 1 if n_groups is None else int(n_groups)
    if G <= grp.max():
        raise ValueError(f"groups holds the label {int(grp.max())}, n_groups is {G}")
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError("max_rounds must be an integer >= 0")
    st = _per_item(start, G, "start", "group")
    if not np.isfinite(st).all():
        raise ValueError("start must be finite")
    pr = _check_prior(GROUP_PRIOR if prior is None else prior, G, "group")
    if not (np.isfinite(pr).all() and (pr[:, 1] > 0).all()):
        raise ValueError("the groups' prior needs finite means and finite sds > 0")
    _check_run_options(storage, chunk_cells)
    prob = _Problem(_keep_genes(counts_U, keep), basis, logm, nu, xy, r, noisemodel, device, chunk_cells, storage)
    const = prob.const.cpu().numpy()

    def evaluate(om):
        out = prob.run(om[grp], None, 0.0, 0)
        ok = out["st"].cpu().numpy() == _lib.VC_CSP_EVALUATED
        return group_sums(out["sums"].cpu().numpy(), out["nc"].cpu().numpy(), ok, grp, G)

    res = solve_groups(evaluate, st, pr[:, 0], 1.0 / pr[:, 1] ** 2, float(tol_outer), int(max_rounds))
    out = prob.run(res["omega"][grp], None, 0.0, 0)                                  # which cells count: those of the last pass
    ok = out["st"].cpu().numpy() == _lib.VC_CSP_EVALUATED
    cst = np.bincount(grp[ok], weights=const[ok], minlength=G)
    cur, none = res["cur"], res["status"] == _lib.VC_CSP_NO_DATA
    nan = lambda v: np.where(none, np.nan, v)                                        # noqa: E731
    pp = 1.0 / pr[:, 1] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return GroupSpeedFit(omega=nan(res["omega"]), stds=nan(1.0 / np.sqrt(cur[:, 2] + pp)), var=nan(1.0 / res["A"]),
                             loglik=nan(cur[:, 0] + cst), score=nan(cur[:, 1]), fisher=nan(cur[:, 2]), observed=nan(cur[:, 3]),
                             dec=nan(res["dec"]), rounds=res["rounds"], status=res["status"], n_cells=res["n_cells"].astype(np.int32),
                             n_clamped=np.where(none, 0, res["n_clamped"]).astype(np.int32))


def phase_bin_groups(directions, bins, condition_design=None):
    """The usual grouping, phase bin within condition: (groups int64 [Nc], centres float64 [bins]) with groups[c] = x bins + j for a cell of
    condition x whose phase lies in [2 pi j / bins, 2 pi (j + 1) / bins) (the phase is the direction's angle in [0, 2 pi)), and
    centres[j] = 2 pi (j + 1/2) / bins.  condition_design: [Nx, Nc] one-hot (every cell in exactly one condition) or None (one)."""
    xy = np.asarray(directions, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[0] != 2:
        raise ValueError(f"directions must be [2, cells] like Phases.phi_xy, got {xy.shape}")
    if int(bins) != bins or bins < 1:
        raise ValueError("bins must be an integer >= 1")
    bins, Nc = int(bins), xy.shape[1]
    if not (np.isfinite(xy).all() and ((xy ** 2).sum(0) > 0).all()):
        raise ValueError("every cell needs a finite phase direction of non-zero length")
    phi = np.mod(np.arctan2(xy[1], xy[0]), 2 * np.pi)
    j = np.minimum((phi / (2 * np.pi) * bins).astype(np.int64), bins - 1)
    x = np.zeros(Nc, dtype=np.int64)
    if condition_design is not None:
        D = np.asarray(condition_design, dtype=np.float64)
        if D.ndim != 2 or D.shape[1] != Nc or D.shape[0] < 1:
            raise ValueError(f"condition_design must be [conditions, cells] = (Nx, {Nc}), got {D.shape}")
        if not (((D == 0) | (D == 1)).all() and (D.sum(0) == 1).all()):
            raise ValueError("condition_design must be one-hot: every cell in exactly one condition")
        x = D.argmax(0).astype(np.int64)
    return x * bins + j, 2 * np.pi * (np.arange(bins) + 0.5) / bins
