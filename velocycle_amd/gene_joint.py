"""The V-joint configuration solved deterministically on the HIP kernel `vc_gene_joint`: per gene the harmonics ν, log γ and log β
estimated together from the spliced AND the unspliced counts at a given angular speed (`gene_joint`), and the MAP angular speed νω with
all of them profiled out (`velocity_map_joint`, the worker behind `AngularSpeed.from_joint_mle` and `Cycle.from_joint_mle`).

The model is the reference's velocity stage conditioned on ϕxy (velocity_inference_model.py:360-386, with_delta_nu=False):

    etaS = nu_g . zeta(phi_c) + a log n_c,   d = nu_g . d zeta / d phi (phi_c),   omega_c = sum_i νω_i W_i(c)
    z = omega_c d + gamma_g,   mu_S = exp(etaS),   mu_U = exp(etaS) (relu(z) + 1e-5) / beta_g
    S ~ Poisson(mu_S) | NegativeBinomial(mu_S, r),   U ~ the same at mu_U (one r per gene for both layers)
    nu_g ~ Normal(prior_means, prior_stds),   log gamma_g ~ Normal(0, 0.5),   log beta_g ~ Normal(2, 3)

The two-stage route (`Cycle.from_phases_mle`, then `AngularSpeed.from_kinetics_mle`) conditions the kinetics on a ν that has never
seen U; here ν enters the unspliced mean twice (through etaS and through d inside the relu) and is fitted to both layers.  With omega
fixed every gene is a problem of 2 H + 3 parameters, which the kernel solves by a Newton iteration inside one workgroup; νω follows as
in `gene_kinetics.velocity_map`, by a damped Newton iteration over the kernel's score and profile information.  ϕ and ω (or the design
of νω) are conditioned on; the standard errors are Laplace's at the mode; `relu` is the model's, kink included (`n_clamped`).

Genes are independent: both layers are staged in the same chunks, and the result does not depend on the chunk size or the storage
bit for bit.  Cells cannot be cut.  Not here: Δν, H = 3, more than 3 coefficients of νω, Lognormal noise; case weights and the cell
bootstrap are `joint_bootstrap`'s (`gene_joint_weighted`, `velocity_map_joint_bootstrap`).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .gene_harmonics import (_check_cells, _check_run_options, _chunks, _constants, _dispersion_to_r, _open_device, _ptr, _row_sums,
                             _unpack_tri, fourier_basis_from_directions)
from .gene_kinetics import (DEFAULT_PRIOR, EPS32, MAP_STATUS, MAX_OUTER_HALVINGS, GeneKineticsFit, _check_omega, _nuw_prior, _solve_spd,
                            omega_design)
from .phase_mle import NOISEMODELS

HARMONICS = (1, 2)                   # csrc/vc_gene_joint.hip
NU_BOUND, XY_BOUND = 50.0, 30.0      # the kernel's box
DEFAULT_NU_PRIOR = (0.0, 3.0)        # Cycle.trivial_prior's Normal(0, 3)
STATUS = {_lib.VC_JNT_CONVERGED: "CONVERGED", _lib.VC_JNT_ROUNDING: "ROUNDING", _lib.VC_JNT_MAX_ITER: "MAX_ITER",
          _lib.VC_JNT_UNBOUNDED: "UNBOUNDED", _lib.VC_JNT_NO_DATA: "NO_DATA", _lib.VC_JNT_EVALUATED: "EVALUATED"}


@dataclass
class GeneJointFit:
    """Host float64 arrays.  means: [K, Ng] like `Cycle.means`; log_gamma, log_beta: [Ng]; cov: [Ng, K + 2, K + 2] over (ν, log γ,
    log β), the inverse of the matrix the last decrement was formed with (the observed Hessian of the penalised objective where its
    Cholesky factorisation succeeds, else the Fisher matrix; both with the prior precisions); stds: [K + 2, Ng] = sqrt of its diagonal;
    loglik_S, loglik_U: [Ng] the full log-likelihoods of the two layers at the point (without the prior); decrement; iterations,
    status, n_clamped: int32 [Ng] (`STATUS` names the codes; n_clamped = cells with z <= 0 at the point); score_w: [Ng, NW] and
    info_w: [Ng, NW, NW], the score and the profile information of the angular speed's coefficients."""
    means: np.ndarray
    log_gamma: np.ndarray
    log_beta: np.ndarray
    cov: np.ndarray
    stds: np.ndarray
    loglik_S: np.ndarray
    loglik_U: np.ndarray
    decrement: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    n_clamped: np.ndarray
    score_w: np.ndarray
    info_w: np.ndarray
    bootstrap = None                 # `Cycle.from_joint_mle(bootstrap=n)` hangs its GeneJointBootstrap here: an attribute, not a field

    def to_cycle(self, cycle_or_gene_names):
        """A `Cycle` with means, stds, `log_gammas` and `log_betas` set: a copy of the given cycle, or a new one over the gene names."""
        from .containers import Cycle
        K = self.means.shape[0]
        if isinstance(cycle_or_gene_names, Cycle):
            out = cycle_or_gene_names.copy()
            if out.means.shape != self.means.shape:
                raise ValueError(f"the cycle is {out.means.shape}, the fit {self.means.shape}")
            out.means.iloc[:, :] = self.means
            out.stds.iloc[:, :] = self.stds[:K]
        else:
            out = Cycle.from_array(self.means.copy(), self.stds[:K].copy(), gene_names=list(cycle_or_gene_names))
        out.set_log_gammas(np.array(self.log_gamma, dtype=np.float64))
        out.set_log_betas(np.array(self.log_beta, dtype=np.float64))
        return out


@dataclass
class JointVelocityMapFit:
    """`gene_kinetics.VelocityMapFit` of the joint problem.  nu_omega, stds: [2 Hω + 1, Nx] float64 in `AngularSpeed`'s row layout;
    cov: [NW, NW] = J^-1 over the coefficients condition-major; F: the profiled log-posterior (both layers' full log-likelihoods, the
    genes' and νω's Gaussian penalties); dec: the last outer decrement; rounds: outer steps taken; status: one of `MAP_STATUS`;
    n_excluded: genes left out after the first round; included: bool [Ng]; genes: the final `GeneJointFit`."""
    nu_omega: np.ndarray
    stds: np.ndarray
    cov: np.ndarray
    F: float
    dec: float
    rounds: int
    status: str
    n_excluded: int
    included: np.ndarray
    genes: GeneJointFit
    bootstrap = None                 # `AngularSpeed.from_joint_mle(bootstrap=n)` hangs its JointVelocityMapBootstrap here: an attribute, not a field

    def to_cycle(self, cycle_or_gene_names):
        return self.genes.to_cycle(cycle_or_gene_names)


def _start_table(start, K, Ng):
    """start as float64 [Ng, K + 2]: (means [K, Ng], log_gamma [Ng], log_beta [Ng]), or (means, GeneKineticsFit) in either order."""
    if not isinstance(start, (tuple, list)) or len(start) not in (2, 3):
        raise ValueError("start must be (means, log_gamma, log_beta) or (means, GeneKineticsFit)")
    if len(start) == 2:
        kin = [s for s in start if isinstance(s, GeneKineticsFit)]
        rest = [s for s in start if not isinstance(s, GeneKineticsFit)]
        if len(kin) != 1:
            raise ValueError("start must be (means, log_gamma, log_beta) or (means, GeneKineticsFit)")
        start = (rest[0], kin[0].log_gamma, kin[0].log_beta)
    nu, x, y = (np.asarray(v, dtype=np.float64) for v in start)
    if nu.shape != (K, Ng) or x.shape != (Ng,) or y.shape != (Ng,):
        raise ValueError(f"start must be means [{K}, {Ng}], log_gamma [{Ng}] and log_beta [{Ng}], got {nu.shape}, {x.shape}, {y.shape}")
    return np.ascontiguousarray(np.concatenate([nu.T, x[:, None], y[:, None]], 1))


def check_arguments(counts_S, counts_U, directions, n_scounts, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, prior_means=None,
                    prior_stds=None, kinetics_prior=DEFAULT_PRIOR, start=None, evaluate_only=False, tol=1e-10, max_iter=40, **refused):
    """Every refusal that needs no device.  Returns (basis float64 [K, Nc], logm float64 [Nc], r float64 [Ng] or None, prior means
    float64 [Ng, K], prior precisions float64 [Ng, K], kinetics prior float64 [Ng, 4], start float64 [Ng, K + 2] or None)."""
    for name in refused:
        if name in ("batch_design", "delta_nu", "delta_nu_prior"):
            raise NotImplementedError("the joint fit knows no batch offsets (Δν): see gene_batch.gene_harmonics_batched for the spliced layer")
        if name in ("cell_weights", "weights"):
            raise NotImplementedError("the joint fit knows no case weights: vc_gene_joint has no weighted twin yet")
        raise TypeError(f"unexpected argument {name!r}")
    if noisemodel not in NOISEMODELS:
        raise NotImplementedError("Not implemented yet, sorry")
    if int(harmonics) != harmonics or int(harmonics) not in HARMONICS:
        raise ValueError("harmonics must be 1 or 2 (3 are not instantiated, 0 have no velocity)")
    K = 2 * int(harmonics) + 1
    Nc, Ng, xy, n = _check_cells(counts_S, directions, n_scounts, tol, max_iter)
    if len(counts_U.shape) != 2 or tuple(int(v) for v in counts_U.shape) != (Nc, Ng):
        raise ValueError(f"counts_U must be [cells, genes] = ({Nc}, {Ng}) like counts_S, got {tuple(counts_U.shape)}")
    r = _dispersion_to_r(noisemodel, dispersion, Ng)
    if (prior_means is None) != (prior_stds is None):
        raise ValueError("a prior needs both prior_means and prior_stds")
    if prior_means is None:
        prior_means, prior_stds = np.full((K, Ng), DEFAULT_NU_PRIOR[0]), np.full((K, Ng), DEFAULT_NU_PRIOR[1])
    pm, ps = np.asarray(prior_means, dtype=np.float64), np.asarray(prior_stds, dtype=np.float64)
    if pm.shape != (K, Ng) or ps.shape != (K, Ng):
        raise ValueError(f"prior_means and prior_stds must be [2 harmonics + 1, genes] = ({K}, {Ng}), got {pm.shape} and {ps.shape}")
    if not (np.isfinite(pm).all() and np.isfinite(ps).all() and (ps > 0).all()):
        raise ValueError("prior_means must be finite and prior_stds finite and > 0: the joint fit needs a prior on every coefficient")
    if kinetics_prior is None or len(kinetics_prior) != 4:
        raise ValueError("kinetics_prior is (mu_gamma, sd_gamma, mu_beta, sd_beta) of log gamma and log beta")
    cols = []
    for v in kinetics_prior:
        t = np.asarray(v, dtype=np.float64).reshape(-1)
        if t.size not in (1, Ng):
            raise ValueError(f"kinetics_prior's entries must be scalars or one value per gene ({Ng}), got {t.size}")
        cols.append(np.broadcast_to(t, (Ng,)))
    pr = np.ascontiguousarray(np.stack(cols, 1))
    if not (pr[:, 1] > 0).all() or not (pr[:, 3] > 0).all():
        raise ValueError("kinetics_prior's standard deviations must be > 0")
    if evaluate_only and start is None:
        raise ValueError("evaluate_only needs start: the (means, log_gamma, log_beta) to evaluate at")
    st = _start_table(start, K, Ng) if start is not None else None
    basis = fourier_basis_from_directions(xy, int(harmonics))
    logm = float(a) * torch.log(torch.as_tensor(n))
    return basis, logm, r, np.ascontiguousarray(pm.T), np.ascontiguousarray(1.0 / ps.T ** 2), pr, st


def _design(directions, Nc, omega, nu_omega, harmonics_w, condition_design):
    """(W float64 [NW, Nc], nuw float64 [NW]) of a speed per cell (its one row is omega itself) or of coefficients on a design."""
    if (omega is None) == (nu_omega is None):
        raise ValueError("give either omega (per cell) or nu_omega (coefficients on the design of harmonics_w and condition_design)")
    if omega is not None:
        return _check_omega(omega, Nc)[None, :], np.ones(1)
    W64 = omega_design(directions, harmonics_w, condition_design)
    nuw = np.asarray(nu_omega, dtype=np.float64).reshape(-1)
    if nuw.shape != (W64.shape[0],) or not np.isfinite(nuw).all():
        raise ValueError(f"nu_omega must be {W64.shape[0]} finite coefficients (condition-major)")
    return W64, nuw


class _Problem:
    """Both layers staged on the device in the same chunks (kept for every call of an outer iteration) and the kernel's launches."""

    def __init__(self, counts_S, counts_U, basis, logm, r, pm, pp, prior, noisemodel, device, chunk_genes, storage):
        self.lib, self.dev, self.Error = _open_device(device)
        self.Nc, self.Ng, self.K = int(counts_S.shape[0]), int(counts_S.shape[1]), int(basis.shape[0])
        self.D = self.K + 2
        self.noise = _lib.NOISE[noisemodel]
        dev = self.dev
        with torch.cuda.device(dev):
            self.B = basis.to(torch.float32).to(dev).contiguous()
            self.logm = logm.to(torch.float32).to(dev).contiguous()
            self.r = r.to(torch.float32).to(dev).contiguous() if r is not None else None
            r64 = self.r.double() if self.r is not None else None                # the model is the one of the float32 r the kernel reads
            self.pm = torch.as_tensor(pm).to(dev).contiguous()
            self.pp = torch.as_tensor(pp).to(dev).contiguous()
            self.prior = torch.as_tensor(prior).to(dev).contiguous()
            self.const_S = torch.empty(self.Ng, dtype=torch.float64, device=dev)
            self.const_U = torch.empty(self.Ng, dtype=torch.float64, device=dev)
            self.chunks = []
            for (g0, g1, blkS, kS, kindS), (u0, u1, blkU, kU, kindU) in zip(_chunks(counts_S, self.Nc, self.Ng, dev, storage, chunk_genes),
                                                                           _chunks(counts_U, self.Nc, self.Ng, dev, storage, chunk_genes)):
                assert (g0, g1) == (u0, u1)
                rr = r64[g0:g1] if r64 is not None else None
                self.const_S[g0:g1] = _constants(blkS, rr)
                self.const_U[g0:g1] = _constants(blkU, rr)
                if kindS != kindU:                                               # a layer that needs float32 storage takes the other with it
                    kS, kU, kindS = blkS, blkU, _lib.VC_COUNTS_F32
                self.chunks.append((g0, g1, kS, kU, kindS))
                del blkS, blkU

    def run(self, W, nuw, start, tol, max_iter):
        """One launch per chunk at the design W (float32 device [NW, Nc]) and the coefficients nuw (host float64 [NW]).  Returns device
        tensors over all genes: theta [Ng, K + 2], cov [Ng, (K + 2)(K + 3) / 2], lls, llu, dec, it, st, nc, score [Ng, NW],
        info [Ng, NW (NW + 1) / 2]."""
        dev, Ng, NW, D = self.dev, self.Ng, int(W.shape[0]), self.D
        NWH = NW * (NW + 1) // 2
        with torch.cuda.device(dev):
            nuw_d = torch.as_tensor(np.ascontiguousarray(nuw, dtype=np.float64)).to(dev)
            start_d = torch.as_tensor(start).to(dev).contiguous() if start is not None and not torch.is_tensor(start) else start
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)         # noqa: E731
            i32 = lambda: torch.empty(Ng, dtype=torch.int32, device=dev)             # noqa: E731
            out = dict(theta=f64(Ng, D), cov=f64(Ng, D * (D + 1) // 2), lls=f64(Ng), llu=f64(Ng), dec=f64(Ng), it=i32(), st=i32(), nc=i32(),
                       score=f64(Ng, max(NW, 1)), info=f64(Ng, max(NWH, 1)))
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for g0, g1, kS, kU, kind in self.chunks:
                sl = lambda t: _ptr(t[g0:g1]) if t is not None else None             # noqa: E731
                rc = self.lib.vc_gene_joint(_ptr(kS), _ptr(kU), kind, g1 - g0, self.Nc, self.Nc, _ptr(self.B), self.K, _ptr(self.logm),
                                            _ptr(W) if NW else None, NW, _ptr(nuw_d) if NW else None, self.noise, sl(self.r), sl(self.pm),
                                            sl(self.pp), sl(self.prior), sl(start_d), float(tol), int(max_iter), sl(out["theta"]),
                                            sl(out["cov"]), sl(out["lls"]), sl(out["llu"]), sl(out["dec"]), sl(out["it"]), sl(out["st"]),
                                            sl(out["nc"]), sl(out["score"]) if NW else None, sl(out["info"]) if NW else None, stream)
                if rc != _lib.VC_OK:
                    raise self.Error(f"vc_gene_joint failed ({rc}): {self.lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # nuw_d and the slices outlive their launches
            out["score"], out["info"] = out["score"][:, :NW], out["info"][:, :NWH]
        return out

    def penalty(self, theta):
        """The genes' Gaussian penalties at theta [Ng, K + 2], device float64 [Ng]."""
        K, p = self.K, self.prior
        nu = 0.5 * (self.pp * (theta[:, :K] - self.pm) ** 2)
        return _row_sums(nu.contiguous()) + 0.5 * ((theta[:, K] - p[:, 0]) / p[:, 1]) ** 2 + 0.5 * ((theta[:, K + 1] - p[:, 2]) / p[:, 3]) ** 2

    def fit(self, out):
        K, D, NW = self.K, self.D, out["score"].shape[1]
        cov = _unpack_tri(out["cov"], D)
        th = out["theta"]
        return GeneJointFit(means=th[:, :K].T.contiguous().cpu().numpy(), log_gamma=th[:, K].cpu().numpy().copy(),
                            log_beta=th[:, K + 1].cpu().numpy().copy(), cov=cov.cpu().numpy(),
                            stds=torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)).T.contiguous().cpu().numpy(),
                            loglik_S=(out["lls"] + self.const_S).cpu().numpy(), loglik_U=(out["llu"] + self.const_U).cpu().numpy(),
                            decrement=out["dec"].cpu().numpy(), iterations=out["it"].cpu().numpy(), status=out["st"].cpu().numpy(),
                            n_clamped=out["nc"].cpu().numpy(), score_w=out["score"].cpu().numpy().copy(),
                            info_w=_unpack_tri(out["info"], NW).cpu().numpy())


def gene_joint(counts_S, counts_U, directions, n_scounts, omega=None, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *,
               prior_means=None, prior_stds=None, kinetics_prior=DEFAULT_PRIOR, start=None, evaluate_only=False, tol=1e-10, max_iter=40,
               device=None, chunk_genes=None, storage="auto", nu_omega=None, harmonics_w=0, condition_design=None, **refused):
    """(ν, log γ, log β) of every gene at the angular speed `omega` (a scalar or one value per cell), on the HIP kernel `vc_gene_joint`:
    the maximum over all 2 H + 3 of both layers' log-likelihood under Normal priors.  counts_S, counts_U: [Nc, Ng] like AnnData layers
    (numpy, scipy sparse or torch); directions, n_scounts, a, dispersion, device, chunk_genes, storage: as for `gene_harmonics` (same
    staging, chunking and truncation; if either layer needs float32 storage both use it); harmonics: H in {1, 2}.  prior_means,
    prior_stds: [2H+1, Ng] of ν (None: Normal(0, 3), `Cycle.trivial_prior`'s default -- a prior is always there, because without one a
    gene with few cells has no maximum); kinetics_prior = (mu_gamma, sd_gamma, mu_beta, sd_beta), scalars or one value per gene.
    start: (means [2H+1, Ng], log_gamma [Ng], log_beta [Ng]) or (means, GeneKineticsFit) -- the natural use is to polish the two-stage
    fit; a gene whose start is not finite or lies outside the kernel's box starts from the default.  evaluate_only=True makes one pass
    at `start`.  A gene without a count in a layer comes back NO_DATA with NaN outputs.  Returns a `GeneJointFit`; with omega its
    score_w / info_w are those of a common factor on omega, with omega=None the speed is that of the coefficients `nu_omega`
    (condition-major) on the design of `harmonics_w` and `condition_design` (`gene_kinetics.omega_design`), and they are theirs."""
    basis, logm, r, pm, pp, pr, st = check_arguments(counts_S, counts_U, directions, n_scounts, harmonics, a, noisemodel, dispersion,
                                                     prior_means, prior_stds, kinetics_prior, start, evaluate_only, tol, max_iter, **refused)
    W64, nuw = _design(directions, int(counts_S.shape[0]), omega, nu_omega, harmonics_w, condition_design)
    _check_run_options(storage, chunk_genes)
    prob = _Problem(counts_S, counts_U, basis, logm, r, pm, pp, pr, noisemodel, device, chunk_genes, storage)
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        return prob.fit(prob.run(W, nuw, st, tol, 0 if evaluate_only else max_iter))


def velocity_map_joint(counts_S, counts_U, directions, n_scounts, harmonics=1, harmonics_w=0, condition_design=None, a=1,
                       noisemodel="Poisson", dispersion=0.3, *, prior_means=None, prior_stds=None, kinetics_prior=DEFAULT_PRIOR,
                       nuw_prior=None, nuw_start=None, start=None, tol=1e-10, max_iter=40, tol_outer=1e-8, max_rounds=30, device=None,
                       chunk_genes=None, storage="auto", **refused):
    """The MAP angular speed with every gene's (ν, log γ, log β) profiled out over both layers:
    F(νω) = sum_g max f_g(theta; νω) - sum_i (νω_i - m_i)^2 / 2 s_i^2, `gene_kinetics.velocity_map`'s outer iteration restated over
    `vc_gene_joint`'s score and profile information: per round one kernel call per chunk, warm-started from the previous theta; the
    genes' values are summed in float64 by halving; G = sum score - Λ (νω - m), J = sum info + Λ, step = J^-1 G, dec = G . step <=
    tol_outer -> CONVERGED.  A trial point is halved while F drops by more than its rounding (8 eps32 sum_g |L_g|), at most 10 times
    (then STALLED); `max_rounds` steps -> MAX_ROUNDS.  Genes whose first-round status is not CONVERGED or ROUNDING are left out from
    then on (`n_excluded`); one that fails later ends the fit with GENE_FAILED.  start: as `gene_joint`'s, for the first round.
    Returns a `JointVelocityMapFit`."""
    basis, logm, r, pm_nu, pp_nu, pr, st = check_arguments(counts_S, counts_U, directions, n_scounts, harmonics, a, noisemodel, dispersion,
                                                           prior_means, prior_stds, kinetics_prior, start, False, tol, max_iter, **refused)
    W64 = omega_design(directions, harmonics_w, condition_design)
    Nhw = 2 * int(harmonics_w) + 1
    NW, Nx = W64.shape[0], W64.shape[0] // Nhw
    pm, pp = _nuw_prior(nuw_prior, Nx, Nhw)
    if not (tol_outer >= 0):
        raise ValueError("tol_outer must be >= 0")
    if int(max_rounds) != max_rounds or max_rounds < 0:
        raise ValueError("max_rounds must be an integer >= 0")
    nuw = pm.copy() if nuw_start is None else np.asarray(nuw_start, dtype=np.float64).reshape(-1).copy()
    if nuw.shape != (NW,) or not np.isfinite(nuw).all():
        raise ValueError(f"nuw_start must be {NW} finite coefficients (condition-major)")
    _check_run_options(storage, chunk_genes)
    prob = _Problem(counts_S, counts_U, basis, logm, r, pm_nu, pp_nu, pr, noisemodel, device, chunk_genes, storage)
    ok_codes = (_lib.VC_JNT_CONVERGED, _lib.VC_JNT_ROUNDING)
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        zero = torch.zeros((), dtype=torch.float64, device=prob.dev)
        const = prob.const_S + prob.const_U

        def evaluate(v, start, inc):
            o = prob.run(W, v, start, tol, max_iter)
            good = (o["st"] == ok_codes[0]) | (o["st"] == ok_codes[1])
            inc = good if inc is None else inc
            ll = o["lls"] + o["llu"]
            f = torch.where(inc, ll + const - prob.penalty(o["theta"]), zero)
            mag = torch.where(inc, ll.abs(), zero)
            sums = _row_sums(torch.cat([f[None, :], mag[None, :], torch.where(inc[:, None], o["score"], zero).T,
                                        torch.where(inc[:, None], o["info"], zero).T]).contiguous()).cpu().numpy()
            J = np.zeros((NW, NW))
            J[np.tril_indices(NW)] = sums[2 + NW:]
            J = J + np.tril(J, -1).T + np.diag(pp)
            d = v - pm
            return dict(out=o, inc=inc, failed=bool((inc & ~good).any()), F=float(sums[0] - 0.5 * (pp * d * d).sum()),
                        allow=8.0 * EPS32 * float(sums[1]), G=sums[2:2 + NW] - pp * d, J=J)

        cur = evaluate(nuw, st, None)
        inc = cur["inc"]
        n_excluded = int((~inc).sum())
        status, rounds, dec = "MAX_ROUNDS", 0, float("nan")
        if n_excluded == prob.Ng:
            status = "GENE_FAILED"
        else:
            while True:
                step = _solve_spd(cur["J"], cur["G"])
                dec = float(cur["G"] @ step)
                if dec <= tol_outer:
                    status = "CONVERGED"
                    break
                if rounds >= max_rounds:
                    status = "MAX_ROUNDS"
                    break
                t, moved = 1.0, False
                for _ in range(MAX_OUTER_HALVINGS + 1):
                    trial = evaluate(nuw + t * step, cur["out"]["theta"], inc)
                    if trial["failed"]:
                        status = "GENE_FAILED"
                        break
                    if trial["F"] >= cur["F"] - max(cur["allow"], trial["allow"]):
                        nuw, cur, moved = nuw + t * step, trial, True
                        break
                    t *= 0.5
                else:
                    status = "STALLED"
                if not moved:
                    break
                rounds += 1
        assert status in MAP_STATUS
        cov = np.linalg.inv(cur["J"])
        table = lambda v: np.ascontiguousarray(v.reshape(Nx, Nhw).T)                 # noqa: E731
        return JointVelocityMapFit(nu_omega=table(nuw), stds=table(np.sqrt(np.diag(cov))), cov=cov, F=cur["F"], dec=dec, rounds=rounds,
                                   status=status, n_excluded=n_excluded, included=inc.cpu().numpy(), genes=prob.fit(cur["out"]))
