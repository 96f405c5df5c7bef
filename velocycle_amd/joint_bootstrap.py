"""The joint per-gene fit under case weights and the cell bootstrap of its MAP angular speed, on the HIP kernel
`vc_gene_joint_weighted`: `gene_joint_weighted` (R rows of weights per call), `gene_joint_bootstrap` (replicates of the genes at a given
angular speed, behind `Cycle.from_joint_mle(bootstrap=)`) and `velocity_map_joint_bootstrap` (replicates of
`gene_joint.velocity_map_joint`, behind `AngularSpeed.from_joint_mle(bootstrap=)`).

`JointVelocityMapFit.stds` are Laplace standard errors from the Fisher profile information of the assumed noise model: right when that
model is, too narrow when a Poisson fit (the default) meets overdispersed counts.  Replicate b draws a Poisson(1) integer weight per cell
(the draw of `gene_bootstrap.draw_weights`: the same seed resamples the same cells as the other bootstraps) and runs
`velocity_map_joint`'s outer iteration again under those case weights; all replicates iterate side by side, one kernel call per chunk and
round over the rows still iterating, each row at its own trial νω and its own previous θ = (ν, log γ, log β).  In the joint problem a
replicate resamples ν, log γ, log β and νω together: the replicates of the cycle and of the kinetics per gene come with it
(`keep_genes`), from a ν that has seen U.

What the replicates measure is SAMPLING VARIABILITY.  For identified contrasts between conditions -- ln(ω_a / ω_b), the comparison the
method exists for -- their spread validates the Laplace error where the noise model holds and replaces it where it does not.  It is NOT
a replacement for the Laplace width of the absolute ω: that width is limited by the prior of gamma, which fixes the time scale and is
common to all conditions, and resampling cells cannot see it.  Nothing here overwrites `JointVelocityMapFit.stds`.

Limits: the dispersion is not estimated again per replicate; resampling is not stratified; no batch offsets (Δν); H in {1, 2}; at most
3 coefficients of the angular speed; the cells are not sharded; no Lognormal noise.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .gene_harmonics import MAX_WEIGHT_ROWS, _check_run_options, _open_device, _ptr, _row_sums, _unpack_tri, check_weights
from .gene_joint import (GeneJointFit, JointVelocityMapFit, _design, _Problem, check_arguments, velocity_map_joint)
from .gene_kinetics import DEFAULT_PRIOR, EPS32, MAP_STATUS, MAX_OUTER_HALVINGS, _nuw_prior, _row_constants, _solve_spd, omega_design
from .kinetics_bootstrap import MAX_OUTPUT_BYTES, VelocityMapBootstrap

OK_CODES = (_lib.VC_JNT_CONVERGED, _lib.VC_JNT_ROUNDING)


class _WeightedProblem(_Problem):
    """`gene_joint._Problem` (both layers staged once, kept for all rounds) with a float32 table [R, Nc] of case weights and the
    launches of `vc_gene_joint_weighted` over its rows.  `const_S_rows`, `const_U_rows`: the layers' constants under every row's
    weights, float64 [R, Ng] (a row of ones: `const_S`, `const_U` bit for bit)."""

    def __init__(self, counts_S, counts_U, basis, logm, r, pm, pp, prior, noisemodel, device, chunk_genes, storage, weights):
        super().__init__(counts_S, counts_U, basis, logm, r, pm, pp, prior, noisemodel, device, chunk_genes, storage)
        dev = self.dev
        with torch.cuda.device(dev):
            self.Wt = torch.as_tensor(weights).to(torch.float32).to(dev).contiguous()
            W64 = self.Wt.double()
            R = int(W64.shape[0])
            r64 = self.r.double() if self.r is not None else None
            self.const_S_rows = torch.empty((R, self.Ng), dtype=torch.float64, device=dev)
            self.const_U_rows = torch.empty((R, self.Ng), dtype=torch.float64, device=dev)
            for g0, g1, kS, kU, kind in self.chunks:
                rr = r64[g0:g1] if r64 is not None else None
                for k, const in ((kS, self.const_S_rows), (kU, self.const_U_rows)):
                    blk = k if kind == _lib.VC_COUNTS_F32 else (k.to(torch.int32) & 0xFFFF).to(torch.float32)
                    const[:, g0:g1] = _row_constants(blk, rr, W64)
                    del blk

    def run_rows(self, W, nuw, start, tol, max_iter, rows=None, want_cov=True):
        """One `vc_gene_joint_weighted` call per chunk over the rows of the weight table (rows: a device int64 index into it, gathered
        into a compact table; None: all of them, A = their number).  nuw: host float64 [NW] shared by the rows, or [A, NW] one per row;
        start: None, device float64 [Ng, K + 2] shared, or [A, Ng, K + 2].  Returns `run`'s device tensors with a leading row axis
        (cov None when not wanted)."""
        dev, Ng, NW, D = self.dev, self.Ng, int(W.shape[0]), self.D
        NWH, NHD = NW * (NW + 1) // 2, D * (D + 1) // 2
        with torch.cuda.device(dev):
            Wt = self.Wt if rows is None else self.Wt[rows].contiguous()
            A = int(Wt.shape[0])
            nuw_d = torch.as_tensor(np.ascontiguousarray(nuw, dtype=np.float64)).to(dev)
            if start is not None:
                start = (torch.as_tensor(start) if not torch.is_tensor(start) else start).to(dev).contiguous()
            if tuple(nuw_d.shape) not in ((NW,), (A, NW)) or (start is not None and tuple(start.shape) not in ((Ng, D), (A, Ng, D))):
                raise ValueError("the per-row inputs do not match the rows of weights")
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)         # noqa: E731
            i32 = lambda n: torch.empty((A, n), dtype=torch.int32, device=dev)       # noqa: E731
            new = lambda n: dict(theta=f64(A, n, D), cov=f64(A, n, NHD) if want_cov else None, lls=f64(A, n), llu=f64(A, n),     # noqa: E731
                                 dec=f64(A, n), it=i32(n), st=i32(n), nc=i32(n), score=f64(A, n, max(NW, 1)), info=f64(A, n, max(NWH, 1)))
            out = new(Ng)
            at = lambda t, off: C.c_void_p(t.data_ptr() + 8 * off)                   # noqa: E731
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for g0, g1, kS, kU, kind in self.chunks:
                n = g1 - g0
                o = out if n == Ng else new(n)                                       # row b, gene g of a call sits at b * n + g
                sl = lambda t: _ptr(t[g0:g1]) if t is not None else None             # noqa: E731
                st_p, st_s = (None, 0) if start is None else ((sl(start), 0) if start.ndim == 2 else (at(start, g0 * D), Ng * D))
                rc = self.lib.vc_gene_joint_weighted(_ptr(kS), _ptr(kU), kind, n, self.Nc, self.Nc, _ptr(self.B), self.K, _ptr(self.logm),
                                                     _ptr(W) if NW else None, NW, _ptr(nuw_d) if NW else None,
                                                     NW if nuw_d.ndim == 2 else 0, self.noise, sl(self.r), sl(self.pm), sl(self.pp),
                                                     sl(self.prior), _ptr(Wt), A, self.Nc, st_p, st_s, float(tol), int(max_iter),
                                                     _ptr(o["theta"]), _ptr(o["cov"]), _ptr(o["lls"]), _ptr(o["llu"]), _ptr(o["dec"]),
                                                     _ptr(o["it"]), _ptr(o["st"]), _ptr(o["nc"]), _ptr(o["score"]) if NW else None,
                                                     _ptr(o["info"]) if NW else None, stream)
                if rc != _lib.VC_OK:
                    raise self.Error(f"vc_gene_joint_weighted failed ({rc}): {self.lib.vc_last_error(None).decode()}")
                if o is not out:
                    for key, t in o.items():
                        if t is not None:
                            out[key][:, g0:g1] = t
            torch.cuda.current_stream(dev).synchronize()                             # the gathered table and the slices outlive their launches
            out["score"], out["info"] = out["score"][:, :, :NW], out["info"][:, :, :NWH]
        return out

    def penalty_rows(self, theta):
        """The genes' Gaussian penalties at theta [A, Ng, K + 2], device float64 [A, Ng]: `penalty`'s operations per row."""
        K, p, A = self.K, self.prior, theta.shape[0]
        nu = 0.5 * (self.pp * (theta[:, :, :K] - self.pm) ** 2)
        return _row_sums(nu.reshape(A * self.Ng, K).contiguous()).reshape(A, self.Ng) + \
            0.5 * ((theta[:, :, K] - p[:, 0]) / p[:, 1]) ** 2 + 0.5 * ((theta[:, :, K + 1] - p[:, 2]) / p[:, 3]) ** 2

    def fit_rows(self, out, rows=None, squeeze=False):
        """The `GeneJointFit` of `run_rows`' tensors: every array with the leading row axis (squeeze: of the one row, without it)."""
        K, D, NW = self.K, self.D, out["score"].shape[2]
        fits = []
        for b in range(out["theta"].shape[0]):
            th, cov = out["theta"][b], _unpack_tri(out["cov"][b], D)
            w = b if rows is None else int(rows[b])
            fits.append(GeneJointFit(
                means=th[:, :K].T.contiguous().cpu().numpy(), log_gamma=th[:, K].cpu().numpy().copy(), log_beta=th[:, K + 1].cpu().numpy().copy(),
                cov=cov.cpu().numpy(), stds=torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)).T.contiguous().cpu().numpy(),
                loglik_S=(out["lls"][b] + self.const_S_rows[w]).cpu().numpy(), loglik_U=(out["llu"][b] + self.const_U_rows[w]).cpu().numpy(),
                decrement=out["dec"][b].cpu().numpy(), iterations=out["it"][b].cpu().numpy(), status=out["st"][b].cpu().numpy(),
                n_clamped=out["nc"][b].cpu().numpy(), score_w=out["score"][b].cpu().numpy().copy(),
                info_w=_unpack_tri(out["info"][b], NW).cpu().numpy()))
        if squeeze:
            return fits[0]
        return GeneJointFit(**{f: np.stack([getattr(x, f) for x in fits]) for f in GeneJointFit.__dataclass_fields__})


def _weight_table(cell_weights, Nc):
    """(float32 host table [R, Nc], whether the caller gave one row as a vector)."""
    w = cell_weights.detach().cpu() if torch.is_tensor(cell_weights) else cell_weights
    if w is None:
        raise ValueError("cell_weights is required: gene_joint.gene_joint is the unweighted fit")
    vector = np.ndim(w) == 1
    return check_weights(w, Nc, rows=1 if vector else None), vector


def _check_output_bytes(R, Ng, D, NW, cov):
    NWH = NW * (NW + 1) // 2
    if R * Ng * (8 * (D + 3 + NW + NWH + (D * (D + 1) // 2 if cov else 0)) + 4 * 3) > MAX_OUTPUT_BYTES:
        raise ValueError(f"the device outputs of {R} rows of weights x {Ng} genes exceed 1 GiB: fit fewer genes or rows per call")


def gene_joint_weighted(counts_S, counts_U, directions, n_scounts, cell_weights, omega=None, harmonics=1, a=1, noisemodel="Poisson",
                        dispersion=0.3, *, prior_means=None, prior_stds=None, kinetics_prior=DEFAULT_PRIOR, start=None,
                        evaluate_only=False, tol=1e-10, max_iter=40, device=None, chunk_genes=None, storage="auto", nu_omega=None,
                        harmonics_w=0, condition_design=None):
    """`gene_joint.gene_joint` with every cell's contribution multiplied by a case weight, on the HIP kernel `vc_gene_joint_weighted`.
    cell_weights: [Nc], or [R, Nc] for R fits in one call (finite, >= 0; at most 65535 rows); every other argument is `gene_joint`'s.
    Returns a `GeneJointFit`; with [R, Nc] every array has a leading row axis (the convention of `gene_kinetics(cell_weights=)`).  The
    priors are not weighted.  A (row, gene) pair without a weighted count in a layer comes back NO_DATA with NaN outputs; a row of ones
    gives `gene_joint`'s bits."""
    basis, logm, r, pm, pp, pr, st = check_arguments(counts_S, counts_U, directions, n_scounts, harmonics, a, noisemodel, dispersion,
                                                     prior_means, prior_stds, kinetics_prior, start, evaluate_only, tol, max_iter)
    Nc, Ng = int(counts_S.shape[0]), int(counts_S.shape[1])
    W64, nuw = _design(directions, Nc, omega, nu_omega, harmonics_w, condition_design)
    _check_run_options(storage, chunk_genes)
    w_host, vector = _weight_table(cell_weights, Nc)
    _check_output_bytes(w_host.shape[0], Ng, int(basis.shape[0]) + 2, W64.shape[0], True)
    prob = _WeightedProblem(counts_S, counts_U, basis, logm, r, pm, pp, pr, noisemodel, device, chunk_genes, storage, w_host)
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        return prob.fit_rows(prob.run_rows(W, nuw, st, tol, 0 if evaluate_only else max_iter), squeeze=vector)


class _GeneReplicates:
    """What the replicates of the genes carry, shared by `GeneJointBootstrap` and `JointVelocityMapBootstrap`: theta_replicates float64
    [R, Ng, K + 2] (ν, log γ, log β), gene_status int32 [R, Ng] (the kernel's codes) and gene_included bool [R, Ng]."""

    def _rows_ok(self):
        return np.ones(self.theta_replicates.shape[0], dtype=bool)

    def gene_stds(self):
        """[K + 2, Ng]: the standard deviation (ddof 1) of every gene's (ν, log γ, log β) over the ok replicates in which the gene was
        included; NaN below 2 of them."""
        if self.theta_replicates is None:
            raise ValueError("the replicates of the genes were not kept: run with keep_genes=True")
        use = (np.asarray(self.gene_included, dtype=bool) & self._rows_ok()[:, None])[:, :, None]
        th = np.where(use, self.theta_replicates, 0.0)
        n = use.sum(0).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = th.sum(0) / n
            var = (np.where(use, self.theta_replicates - mean, 0.0) ** 2).sum(0) / (n - 1.0)
        return np.ascontiguousarray(np.where(n >= 2, np.sqrt(var), np.nan).T)

    def _cycle_with_stds(self, cycle):
        K = cycle.means.shape[0]
        cycle.stds.iloc[:, :] = self.gene_stds()[:K]
        return cycle


@dataclass
class GeneJointBootstrap(_GeneReplicates):
    """Replicates of `gene_joint` at a given angular speed.  theta_replicates, gene_status, gene_included: see `gene_stds`; fit: the
    full-data `GeneJointFit`; weights: the float32 [R, Nc] table when it was asked for."""
    theta_replicates: np.ndarray
    gene_status: np.ndarray
    gene_included: np.ndarray
    fit: Optional[GeneJointFit] = None
    weights: Optional[np.ndarray] = None

    def to_cycle(self, cycle_or_gene_names):
        """The full-data joint cycle with the bootstrap stds of ν."""
        return self._cycle_with_stds(self.fit.to_cycle(cycle_or_gene_names))


@dataclass
class JointVelocityMapBootstrap(VelocityMapBootstrap, _GeneReplicates):
    """`kinetics_bootstrap.VelocityMapBootstrap` of the joint problem: its fields and summaries (`ok`, `means`, `cov`, `stds`, `bias`,
    `interval`, `contrast`, `contrast_std`, `contrast_interval`) with `fit` the full-data `JointVelocityMapFit`.  With
    `keep_genes=True` also theta_replicates float64 [R, Ng, K + 2] (ν, log γ, log β of every replicate), gene_status int32 [R, Ng] and
    gene_included bool [R, Ng] (False where the replicate left the gene out).  laplace_stds: float64 [R, 2 Hω + 1, Nx], every
    replicate's own Laplace standard errors (sqrt of the diagonal of J^-1 at its last accepted point, `JointVelocityMapFit.stds` of the
    resampled data; NaN where its J has no inverse): what the noise model claims per replicate, next to the spread the replicates show."""
    laplace_stds: Optional[np.ndarray] = None
    theta_replicates: Optional[np.ndarray] = None
    gene_status: Optional[np.ndarray] = None
    gene_included: Optional[np.ndarray] = None

    def _rows_ok(self):
        return self.ok

    def to_cycle(self, cycle_or_gene_names):
        """The full-data joint cycle (`fit.to_cycle`) with the bootstrap stds of ν (`gene_stds`)."""
        return self._cycle_with_stds(self.fit.to_cycle(cycle_or_gene_names))


def _rows_of(n_boot, weights, Nc):
    """(float32 host table or None, R) of a bootstrap's `n_boot` / `weights`."""
    if weights is not None:
        w_host = check_weights(weights.detach().cpu() if torch.is_tensor(weights) else weights, Nc)
        return w_host, int(w_host.shape[0])
    if isinstance(n_boot, bool) or int(n_boot) != n_boot or not 1 <= n_boot <= MAX_WEIGHT_ROWS:
        raise ValueError(f"n_boot must be an integer in 1..{MAX_WEIGHT_ROWS}")
    return None, int(n_boot)


def _table(w_host, R, Nc, seed, device):
    if w_host is not None:
        return w_host
    from .gene_bootstrap import draw_weights
    return draw_weights(R, Nc, seed, _open_device(device)[1])


def _theta_table(genes: GeneJointFit):
    return np.ascontiguousarray(np.concatenate([genes.means.T, genes.log_gamma[:, None], genes.log_beta[:, None]], 1), dtype=np.float64)


def gene_joint_bootstrap(counts_S, counts_U, directions, n_scounts, omega=None, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *,
                         n_boot=200, seed=0, weights=None, fit=None, warm_start=True, return_weights=False, prior_means=None,
                         prior_stds=None, kinetics_prior=DEFAULT_PRIOR, tol=1e-10, max_iter=40, device=None, chunk_genes=None,
                         storage="auto", nu_omega=None, harmonics_w=0, condition_design=None):
    """`n_boot` cell bootstrap replicates of `gene_joint` at a given angular speed: one `vc_gene_joint_weighted` call per chunk over all
    rows of `gene_bootstrap.draw_weights(n_boot, Nc, seed, dev)` (or the caller's [R, Nc] `weights`).  fit: the full-data `GeneJointFit`
    (None: `gene_joint` is run first); warm_start: every replicate starts at it.  A replicate includes the genes that end CONVERGED /
    ROUNDING under its weights.  Returns a `GeneJointBootstrap`."""
    if isinstance(dispersion, str):
        raise ValueError(f"the bootstrap does not support dispersion={dispersion!r}: vc_gene_dispersion knows no weights; hand over the "
                         "estimated dispersions instead")
    basis, logm, r, pm, pp, pr, _ = check_arguments(counts_S, counts_U, directions, n_scounts, harmonics, a, noisemodel, dispersion,
                                                    prior_means, prior_stds, kinetics_prior, None, False, tol, max_iter)
    Nc, Ng, K = int(counts_S.shape[0]), int(counts_S.shape[1]), int(basis.shape[0])
    W64, nuw = _design(directions, Nc, omega, nu_omega, harmonics_w, condition_design)
    _check_run_options(storage, chunk_genes)
    w_host, R = _rows_of(n_boot, weights, Nc)
    _check_output_bytes(R, Ng, K + 2, W64.shape[0], False)
    if fit is not None and (np.shape(fit.means), np.shape(fit.log_gamma)) != ((K, Ng), (Ng,)):
        raise ValueError(f"fit must be the GeneJointFit of this problem: means [{K}, {Ng}]; got {np.shape(fit.means)}")
    if fit is None:
        from .gene_joint import gene_joint
        fit = gene_joint(counts_S, counts_U, directions, n_scounts, omega, harmonics, a, noisemodel, dispersion, prior_means=prior_means,
                         prior_stds=prior_stds, kinetics_prior=kinetics_prior, tol=tol, max_iter=max_iter, device=device,
                         chunk_genes=chunk_genes, storage=storage, nu_omega=nu_omega, harmonics_w=harmonics_w,
                         condition_design=condition_design)
    prob = _WeightedProblem(counts_S, counts_U, basis, logm, r, pm, pp, pr, noisemodel, device, chunk_genes, storage,
                            _table(w_host, R, Nc, seed, device))
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        o = prob.run_rows(W, nuw, torch.as_tensor(_theta_table(fit)).to(prob.dev) if warm_start else None, tol, max_iter, want_cov=False)
        st = o["st"].cpu().numpy()
        return GeneJointBootstrap(theta_replicates=o["theta"].cpu().numpy(), gene_status=st, gene_included=np.isin(st, OK_CODES), fit=fit,
                                  weights=prob.Wt.cpu().numpy() if return_weights else None)


def check_bootstrap_arguments(Nc, Ng, K, NW, Nhw, n_boot, weights, fit):
    """The refusals of `velocity_map_joint_bootstrap` that need no device.  Returns (the float32 host table or None, R)."""
    w_host, R = _rows_of(n_boot, weights, Nc)
    _check_output_bytes(R, Ng, K + 2, NW, False)
    if fit is not None:
        if not isinstance(fit, JointVelocityMapFit):
            raise ValueError("fit must be the JointVelocityMapFit of this problem (gene_joint.velocity_map_joint)")
        shapes = (np.shape(fit.nu_omega), np.shape(fit.included), np.shape(fit.genes.means), np.shape(fit.genes.log_gamma))
        if shapes != ((Nhw, NW // Nhw), (Ng,), (K, Ng), (Ng,)):
            raise ValueError(f"fit must be the JointVelocityMapFit of this problem: nu_omega [{Nhw}, {NW // Nhw}], included [{Ng}] and "
                             f"genes.means [{K}, {Ng}]; got {shapes}")
    return w_host, R


def velocity_map_joint_bootstrap(counts_S, counts_U, directions, n_scounts, harmonics=1, harmonics_w=0, condition_design=None, a=1,
                                 noisemodel="Poisson", dispersion=0.3, *, n_boot=200, seed=0, weights=None, fit=None, warm_start=True,
                                 keep_genes=False, return_weights=False, prior_means=None, prior_stds=None, kinetics_prior=DEFAULT_PRIOR,
                                 nuw_prior=None, nuw_start=None, tol=1e-10, max_iter=40, tol_outer=1e-8, max_rounds=30, device=None,
                                 chunk_genes=None, storage="auto"):
    """counts_S, counts_U, directions, n_scounts, harmonics, harmonics_w, condition_design, a, noisemodel, dispersion (a number or one per
    gene), prior_means, prior_stds, kinetics_prior, nuw_prior, nuw_start, tol, max_iter, tol_outer, max_rounds, device, chunk_genes,
    storage: as for `velocity_map_joint`.  Returns a `JointVelocityMapBootstrap` of `n_boot` replicates of the MAP angular speed.

    weights=None: the table is `gene_bootstrap.draw_weights(n_boot, Nc, seed, dev)`, a pure function of (seed, b, c): the same seed
    resamples the same cells as `gene_harmonics_bootstrap` and `velocity_map_bootstrap`, and the first 2 rows of a 4-row run are the
    2-row run's.  weights=[R, Nc]: the caller's table (finite, >= 0; n_boot is then R).  fit: the full-data `JointVelocityMapFit` (None:
    `velocity_map_joint` is run first with the same arguments); it is returned as `.fit`.  warm_start: every replicate starts at `fit`'s
    νω and at `fit.genes`' θ (False: at `nuw_start` or the prior means and the kernel's default start, as `velocity_map_joint` does).

    The outer iteration is `velocity_map_joint`'s, per row: G, J, the step, the decrement, the halving (at most 10), `max_rounds` and
    the statuses are its own rules, the genes' values summed per row by halving.  A replicate leaves out the genes `fit` left out and
    those whose first-round status under its weights is not CONVERGED / ROUNDING.  A replicate whose J is not positive definite ends
    STALLED.  A replicate's result is a function of its weight row and its starts alone: not of R, of the other rows or of the
    chunking.  keep_genes: also return every replicate's θ, kernel status and included genes (`gene_stds`, `to_cycle`);
    return_weights: the table.

    tol_outer: `velocity_map_joint` has no rounding rule in its outer iteration and neither has this: where the float32 sums of a large
    problem (50 000 x 2 000) do not resolve the default 1e-8, replicates sit just above it until `max_rounds` and end MAX_ROUNDS; the
    summaries over the CONVERGED ones are then a biased selection.  A RuntimeWarning says so; 1e-6 (a thousandth of a standard error)
    is safe there.

    Refused: `dispersion` as a string (`vc_gene_dispersion` knows no weights), n_boot outside 1..65535, device outputs above 1 GiB,
    shapes that do not match, a `fit` of another problem -- all before any device work.  What the replicates mean, and what they do
    not: the module's docstring."""
    if isinstance(dispersion, str):
        raise ValueError(f"the bootstrap does not support dispersion={dispersion!r}: vc_gene_dispersion knows no weights; hand over the "
                         "estimated dispersions instead")
    basis, logm, r, pm_nu, pp_nu, pr, _ = check_arguments(counts_S, counts_U, directions, n_scounts, harmonics, a, noisemodel, dispersion,
                                                          prior_means, prior_stds, kinetics_prior, None, False, tol, max_iter)
    W64 = omega_design(directions, harmonics_w, condition_design)
    Nhw = 2 * int(harmonics_w) + 1
    NW, Nx = W64.shape[0], W64.shape[0] // Nhw
    pm, pp = _nuw_prior(nuw_prior, Nx, Nhw)
    if not (tol_outer >= 0):
        raise ValueError("tol_outer must be >= 0")
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError("max_rounds must be an integer >= 0")
    first = pm.copy() if nuw_start is None else np.asarray(nuw_start, dtype=np.float64).reshape(-1).copy()
    if first.shape != (NW,) or not np.isfinite(first).all():
        raise ValueError(f"nuw_start must be {NW} finite coefficients (condition-major)")
    _check_run_options(storage, chunk_genes)
    Nc, Ng, K = int(counts_S.shape[0]), int(counts_S.shape[1]), int(basis.shape[0])
    w_host, R = check_bootstrap_arguments(Nc, Ng, K, NW, Nhw, n_boot, weights, fit)
    if fit is None:
        fit = velocity_map_joint(counts_S, counts_U, directions, n_scounts, harmonics, harmonics_w, condition_design, a, noisemodel,
                                 dispersion, prior_means=prior_means, prior_stds=prior_stds, kinetics_prior=kinetics_prior,
                                 nuw_prior=nuw_prior, nuw_start=nuw_start, tol=tol, max_iter=max_iter, tol_outer=tol_outer,
                                 max_rounds=max_rounds, device=device, chunk_genes=chunk_genes, storage=storage)
    prob = _WeightedProblem(counts_S, counts_U, basis, logm, r, pm_nu, pp_nu, pr, noisemodel, device, chunk_genes, storage,
                            _table(w_host, R, Nc, seed, device))
    dev = prob.dev
    M = 2 + NW + NW * (NW + 1) // 2
    with torch.cuda.device(dev):
        W = torch.as_tensor(W64).to(torch.float32).to(dev).contiguous()
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        base = torch.as_tensor(np.asarray(fit.included, dtype=bool)).to(dev)[None, :].expand(R, Ng)
        const = prob.const_S_rows + prob.const_U_rows

        def evaluate(idx, V, start, inc):
            """The rows idx (ascending) at their coefficients V [A, NW]: per row what `velocity_map_joint`'s evaluate returns."""
            rows = None if len(idx) == R else torch.as_tensor(idx, device=dev)
            take = (lambda t: t) if rows is None else (lambda t: t[rows])
            o = prob.run_rows(W, V, start, tol, max_iter, rows=rows, want_cov=False)
            good = (o["st"] == OK_CODES[0]) | (o["st"] == OK_CODES[1])
            inc = (good & take(base)) if inc is None else inc
            ll = o["lls"] + o["llu"]
            f = torch.where(inc, ll + take(const) - prob.penalty_rows(o["theta"]), zero)
            mag = torch.where(inc, ll.abs(), zero)
            parts = torch.cat([f[:, None, :], mag[:, None, :], torch.where(inc[:, :, None], o["score"], zero).transpose(1, 2),
                               torch.where(inc[:, :, None], o["info"], zero).transpose(1, 2)], 1)
            sums = _row_sums(parts.reshape(-1, Ng).contiguous()).reshape(len(idx), M).cpu().numpy()
            failed = (inc & ~good).any(1).cpu().numpy()
            res = []
            for j in range(len(idx)):
                J = np.zeros((NW, NW))
                J[np.tril_indices(NW)] = sums[j, 2 + NW:]
                J = J + np.tril(J, -1).T + np.diag(pp)
                d = V[j] - pm
                res.append(dict(failed=bool(failed[j]), F=float(sums[j, 0] - 0.5 * (pp * d * d).sum()), allow=8.0 * EPS32 * float(sums[j, 1]),
                                G=sums[j, 2:2 + NW] - pp * d, J=J))
            return o, inc, res

        every = np.arange(R)
        if warm_start:
            nuw = np.tile(np.ascontiguousarray(np.asarray(fit.nu_omega, dtype=np.float64).T).reshape(-1), (R, 1))
            start = torch.as_tensor(_theta_table(fit.genes)).to(dev)
        else:
            nuw, start = np.tile(first, (R, 1)), None
        o, inc, cur = evaluate(every, nuw, start, None)
        theta, st = o["theta"].clone(), o["st"].clone()
        n_excluded = (~inc).sum(1).cpu().numpy()
        status = np.array(["MAX_ROUNDS"] * R, dtype=object)
        rounds, dec = np.zeros(R, dtype=np.int64), np.full(R, np.nan)
        step, t, halved = np.zeros((R, NW)), np.ones(R), np.zeros(R, dtype=np.int64)
        active = np.ones(R, dtype=bool)

        def finish(b, word):
            status[b], active[b] = word, False

        def next_trial(b):
            """`velocity_map_joint`'s head of a round for row b: the step and its decrement, or the end of the row."""
            try:
                step[b] = _solve_spd(cur[b]["J"], cur[b]["G"])
            except np.linalg.LinAlgError:
                return finish(b, "STALLED")
            dec[b] = float(cur[b]["G"] @ step[b])
            if dec[b] <= tol_outer:
                return finish(b, "CONVERGED")
            if rounds[b] >= max_rounds:
                return finish(b, "MAX_ROUNDS")
            t[b], halved[b] = 1.0, 0

        for b in every:
            if n_excluded[b] == Ng:
                finish(b, "GENE_FAILED")
            else:
                next_trial(b)
        while active.any():
            idx = np.flatnonzero(active)
            V = np.stack([nuw[b] + t[b] * step[b] for b in idx])
            rows = torch.as_tensor(idx, device=dev)
            o, _, trial = evaluate(idx, V, theta[rows], inc[rows])
            moved = []
            for j, b in enumerate(idx):
                if trial[j]["failed"]:
                    finish(b, "GENE_FAILED")
                elif trial[j]["F"] >= cur[b]["F"] - max(cur[b]["allow"], trial[j]["allow"]):
                    nuw[b], cur[b] = V[j], trial[j]
                    moved.append(j)
                    rounds[b] += 1
                    next_trial(b)
                else:
                    t[b] *= 0.5
                    halved[b] += 1
                    if halved[b] > MAX_OUTER_HALVINGS:
                        finish(b, "STALLED")
            if moved:
                src = torch.as_tensor(np.asarray(moved), device=dev)
                theta[rows[src]], st[rows[src]] = o["theta"][src], o["st"][src]
        assert set(status) <= set(MAP_STATUS)
        late = status == "MAX_ROUNDS"
        if max_rounds > 0 and late.any():                  # the summaries run over the CONVERGED rows: a selection, when the others only missed tol_outer
            warnings.warn(f"{int(late.sum())} of {R} replicates took max_rounds = {max_rounds} steps without reaching tol_outer = {tol_outer:g} "
                          f"(their last decrements: {np.nanmin(dec[late]):.3g} .. {np.nanmax(dec[late]):.3g}).  Where these are small the float32 "
                          "sums of this problem do not resolve tol_outer and the converged replicates are a biased selection: raise tol_outer "
                          "(1e-6 is a thousandth of a standard error)", RuntimeWarning, stacklevel=2)
        table = nuw.reshape(R, Nx, Nhw).transpose(0, 2, 1)
        laplace = np.full((R, NW), np.nan)
        for b in every:
            try:
                laplace[b] = np.sqrt(np.diag(np.linalg.inv(cur[b]["J"])))
            except np.linalg.LinAlgError:
                pass
        genes = dict(theta_replicates=theta.cpu().numpy().copy(), gene_status=st.cpu().numpy(),
                     gene_included=inc.cpu().numpy().copy()) if keep_genes else {}
        return JointVelocityMapBootstrap(nu_omega_replicates=np.ascontiguousarray(table), status=status.astype(str), rounds=rounds,
                                         n_excluded=n_excluded.astype(np.int64), F=np.array([c["F"] for c in cur]), dec=dec, fit=fit,
                                         weights=prob.Wt.cpu().numpy() if return_weights else None,
                                         laplace_stds=np.ascontiguousarray(laplace.reshape(R, Nx, Nhw).transpose(0, 2, 1)), **genes)
