"""The velocity half of the model solved deterministically on the HIP kernel `vc_gene_kinetics`: per-gene kinetics (log gamma, log beta)
at a given angular speed (`gene_kinetics`), and the MAP angular speed νω with the kinetics profiled out (`velocity_map`, the worker
behind `AngularSpeed.from_kinetics_mle`).  With case weights per cell (`cell_weights=`) both run on `vc_gene_kinetics_weighted`; the
cell bootstrap built on it is `kinetics_bootstrap.velocity_map_bootstrap`.

The model is the reference's velocity stage conditioned on ϕxy and ν (velocity_inference_model.py:360-386, with_delta_nu=False):

    etaS = nu_g . zeta(phi_c) + a log n_c,   d = nu_g . d zeta / d phi (phi_c),   omega_c = sum_i νω_i W_i(c)
    z = omega_c d + gamma_g,   mu_U = exp(etaS) (relu(z) + 1e-5) / beta_g,   U ~ Poisson(mu_U) | NegativeBinomial(mu_U, r)
    log gamma_g ~ Normal(0, 0.5),   log beta_g ~ Normal(2, 3),   νω ~ the Normals of an `AngularSpeed`

With omega fixed every gene is a two-parameter problem, which the kernel solves by a Newton iteration inside one workgroup; the
derivative of the profiled objective F(νω) = sum_g max_(x, y) f_g with respect to νω is the kernel's score (envelope theorem), its
curvature the kernel's profile information, so νω follows by a damped Newton iteration of a handful of kernel calls on the host.
`relu` makes f_g non-concave where cells have z <= 0 (`n_clamped` counts them): the fit is the model's, kink included.

Genes are independent: they are staged in chunks exactly as `gene_harmonics` stages them, and the result does not depend on the chunk
size, the storage or the layer's format bit for bit.  Cells cannot be cut.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .gene_harmonics import (_check_cells, _check_run_options, _chunks, _constants, _dispersion_to_r, _open_device, _ptr, _row_sums,
                             _unpack_tri, check_weights, fourier_basis_from_directions)
from .phase_mle import NOISEMODELS

HARMONICS = (1, 2)                   # csrc/vc_gene_kinetics.hip
MAX_NW = 3
DEFAULT_PRIOR = (0.0, 0.5, 2.0, 3.0)  # mu_gamma, sd_gamma, mu_beta, sd_beta: the model's
EPS32 = float(np.finfo(np.float32).eps)
STATUS = {_lib.VC_KIN_CONVERGED: "CONVERGED", _lib.VC_KIN_ROUNDING: "ROUNDING", _lib.VC_KIN_MAX_ITER: "MAX_ITER",
          _lib.VC_KIN_UNBOUNDED: "UNBOUNDED", _lib.VC_KIN_NO_DATA: "NO_DATA", _lib.VC_KIN_EVALUATED: "EVALUATED"}
MAP_STATUS = ("CONVERGED", "STALLED", "MAX_ROUNDS", "GENE_FAILED")
MAX_OUTER_HALVINGS = 10


def _with_kinetics(cycle, log_gamma, log_beta):
    out = cycle.copy()
    out.set_log_gammas(np.array(log_gamma, dtype=np.float64))
    out.set_log_betas(np.array(log_beta, dtype=np.float64))
    return out


@dataclass
class GeneKineticsFit:
    """Host float64 arrays.  log_gamma, log_beta: [Ng]; cov: [Ng, 2, 2], the inverse of the matrix the last decrement was formed with
    (the observed Hessian of the penalised objective where it is positive definite, else the Fisher matrix; both with the prior
    precisions); stds: [2, Ng] = sqrt of its diagonal; loglik: [Ng] the full log-likelihood of the unspliced counts at the point
    (without the prior); decrement; iterations, status, n_clamped: int32 [Ng] (`STATUS` names the codes; n_clamped = cells with
    z <= 0 at the point); score_w: [Ng, NW] and info_w: [Ng, NW, NW], the score and the profile information of the angular speed's
    coefficients.  A fit under several rows of case weights (`cell_weights` [R, Nc]) has a leading row axis on every array."""
    log_gamma: np.ndarray
    log_beta: np.ndarray
    cov: np.ndarray
    stds: np.ndarray
    loglik: np.ndarray
    decrement: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    n_clamped: np.ndarray
    score_w: np.ndarray
    info_w: np.ndarray

    def to_cycle(self, cycle):
        """A copy of `cycle` with `log_gammas` and `log_betas` set."""
        return _with_kinetics(cycle, self.log_gamma, self.log_beta)


@dataclass
class VelocityMapFit:
    """nu_omega, stds: [2 Hω + 1, Nx] float64 in `AngularSpeed`'s row layout; cov: [NW, NW] = J^-1 over the coefficients in the order
    condition-major (i = x (2 Hω + 1) + h); F: the profiled log-posterior (full log-likelihood, the genes' and νω's Gaussian penalties);
    dec: the last outer decrement; rounds: outer steps taken; status: one of `MAP_STATUS`; n_excluded: genes left out after the first
    round; included: bool [Ng]; kinetics: the final `GeneKineticsFit`."""
    nu_omega: np.ndarray
    stds: np.ndarray
    cov: np.ndarray
    F: float
    dec: float
    rounds: int
    status: str
    n_excluded: int
    included: np.ndarray
    kinetics: GeneKineticsFit
    bootstrap = None                 # `AngularSpeed.from_kinetics_mle(bootstrap=n)` hangs its VelocityMapBootstrap here: an attribute, not a field

    def to_cycle(self, cycle):
        """A copy of `cycle` with `log_gammas` and `log_betas` set."""
        return self.kinetics.to_cycle(cycle)


def check_arguments(counts, directions, n_scounts, means, a=1, noisemodel="Poisson", dispersion=0.3, prior=DEFAULT_PRIOR, start=None,
                    evaluate_only=False, tol=1e-10, max_iter=25):
    """Every refusal that needs no device.  Returns (basis float64 [K, Nc], logm float64 [Nc], nu float64 [Ng, K], r float64 [Ng] or
    None, prior float64 [Ng, 4], start float64 [Ng, 2] or None)."""
    if noisemodel not in NOISEMODELS:
        raise NotImplementedError("Not implemented yet, sorry")
    nu = np.asarray(means, dtype=np.float64)
    if nu.ndim != 2 or nu.shape[0] not in (3, 5):
        raise ValueError(f"means must be [2 harmonics + 1, genes] with 1 or 2 harmonics (3 are not instantiated, 0 have no velocity), "
                         f"got {nu.shape}")
    Nc, Ng, xy, n = _check_cells(counts, directions, n_scounts, tol, max_iter)
    if nu.shape[1] != Ng:
        raise ValueError(f"means has {nu.shape[1]} genes, counts {Ng}")
    r = _dispersion_to_r(noisemodel, dispersion, Ng)
    if prior is None or len(prior) != 4:
        raise ValueError("the prior is (mu_gamma, sd_gamma, mu_beta, sd_beta) of log gamma and log beta")
    cols = []
    for v in prior:
        t = np.asarray(v, dtype=np.float64).reshape(-1)
        if t.size not in (1, Ng):
            raise ValueError(f"the prior's entries must be scalars or one value per gene ({Ng}), got {t.size}")
        cols.append(np.broadcast_to(t, (Ng,)))
    pr = np.ascontiguousarray(np.stack(cols, 1))
    if not (pr[:, 1] > 0).all() or not (pr[:, 3] > 0).all():
        raise ValueError("the prior's standard deviations must be > 0")
    if evaluate_only and start is None:
        raise ValueError("evaluate_only needs start: the (log gamma, log beta) to evaluate at")
    st = None
    if start is not None:
        st = np.asarray(start, dtype=np.float64)
        if st.shape != (2, Ng):
            raise ValueError(f"start must be [2, genes] = (2, {Ng}): rows log gamma, log beta; got {st.shape}")
        st = np.ascontiguousarray(st.T)
    basis = fourier_basis_from_directions(xy, (nu.shape[0] - 1) // 2)
    logm = float(a) * torch.log(torch.as_tensor(n))
    return basis, logm, np.ascontiguousarray(nu.T), r, pr, st


def _check_omega(omega, Nc):
    om = np.asarray(omega, dtype=np.float64).reshape(-1)
    if om.size == 1:
        om = np.broadcast_to(om, (Nc,))
    if om.size != Nc:
        raise ValueError(f"omega must be a scalar or one value per cell ({Nc}), got {om.size}")
    if not np.isfinite(om).all():
        raise ValueError("omega must be finite")
    return np.ascontiguousarray(om)


def _row_constants(blk, r64, W64):
    """`_constants(blk, r64, W64[b])` of every row b of the float64 weights W64 [R, Nc], float64 [R, n]: each cell's term is formed once
    and multiplied by every row in turn -- the same operations in the same order as `_constants`, so the same bits (ones change none)."""
    out = torch.empty((W64.shape[0], blk.shape[0]), dtype=torch.float64, device=blk.device)
    rows = max(1, (1 << 24) // blk.shape[1])
    for i in range(0, blk.shape[0], rows):
        k = blk[i:i + rows].double()
        t = -torch.lgamma(k + 1.0)
        if r64 is not None:
            rr = r64[i:i + rows, None]
            t += torch.lgamma(k + rr) - torch.lgamma(rr)
        for b in range(W64.shape[0]):
            out[b, i:i + rows] = _row_sums(t * W64[b][None, :])
    return out


class _Problem:
    """The genes staged on the device in chunks (kept for every call of an outer iteration) and the kernel's launches over them.
    weights: None, or the float32 table [R, Nc] of case weights (host or device) `run_rows` solves under; `const` is then [R, Ng]."""

    def __init__(self, counts, basis, logm, nu, r, prior, noisemodel, device, chunk_genes, storage, weights=None):
        self.lib, self.dev, self.Error = _open_device(device)
        self.Nc, self.Ng, self.K = int(counts.shape[0]), int(counts.shape[1]), int(basis.shape[0])
        self.noise = _lib.NOISE[noisemodel]
        dev = self.dev
        with torch.cuda.device(dev):
            self.B = basis.to(torch.float32).to(dev).contiguous()
            self.logm = logm.to(torch.float32).to(dev).contiguous()
            self.nu = torch.as_tensor(nu).to(dev).contiguous()
            self.r = r.to(torch.float32).to(dev).contiguous() if r is not None else None
            r64 = self.r.double() if self.r is not None else None                # the model is the one of the float32 r the kernel reads
            self.prior = torch.as_tensor(prior).to(dev).contiguous()
            self.Wt = torch.as_tensor(weights).to(torch.float32).to(dev).contiguous() if weights is not None else None
            W64 = self.Wt.double() if self.Wt is not None else None
            self.const = torch.empty(self.Ng if W64 is None else (W64.shape[0], self.Ng), dtype=torch.float64, device=dev)
            self.chunks = []
            for g0, g1, blk, kblk, kind in _chunks(counts, self.Nc, self.Ng, dev, storage, chunk_genes):
                rr = r64[g0:g1] if r64 is not None else None
                if W64 is None:
                    self.const[g0:g1] = _constants(blk, rr)
                elif W64.shape[0] == 1:
                    self.const[0, g0:g1] = _constants(blk, rr, W64[0])
                else:
                    self.const[:, g0:g1] = _row_constants(blk, rr, W64)
                self.chunks.append((g0, g1, kblk, kind))
                del blk

    def run(self, W, nuw, start, tol, max_iter):
        """One launch per chunk at the design W (float32 device [NW, Nc]) and the coefficients nuw (host float64 [NW]).  Returns device
        tensors over all genes: xy [Ng, 2], cov [Ng, 3], ll, dec, it, st, nc, score [Ng, NW], info [Ng, NW (NW + 1) / 2]."""
        dev, Ng, NW = self.dev, self.Ng, int(W.shape[0])
        NWH = NW * (NW + 1) // 2
        with torch.cuda.device(dev):
            nuw_d = torch.as_tensor(np.ascontiguousarray(nuw, dtype=np.float64)).to(dev)
            start_d = torch.as_tensor(start).to(dev).contiguous() if start is not None and not torch.is_tensor(start) else start
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)         # noqa: E731
            i32 = lambda: torch.empty(Ng, dtype=torch.int32, device=dev)             # noqa: E731
            out = dict(xy=f64(Ng, 2), cov=f64(Ng, 3), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32(), nc=i32(), score=f64(Ng, max(NW, 1)),
                       info=f64(Ng, max(NWH, 1)))
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for g0, g1, kblk, kind in self.chunks:
                sl = lambda t: _ptr(t[g0:g1]) if t is not None else None             # noqa: E731
                rc = self.lib.vc_gene_kinetics(_ptr(kblk), kind, g1 - g0, self.Nc, self.Nc, _ptr(self.B), self.K, _ptr(self.logm),
                                               sl(self.nu), _ptr(W) if NW else None, NW, _ptr(nuw_d) if NW else None, self.noise,
                                               sl(self.r), sl(self.prior), sl(start_d), float(tol), int(max_iter), sl(out["xy"]),
                                               sl(out["cov"]), sl(out["ll"]), sl(out["dec"]), sl(out["it"]), sl(out["st"]), sl(out["nc"]),
                                               sl(out["score"]) if NW else None, sl(out["info"]) if NW else None, stream)
                if rc != _lib.VC_OK:
                    raise self.Error(f"vc_gene_kinetics failed ({rc}): {self.lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # nuw_d and the slices outlive their launches
            out["score"], out["info"] = out["score"][:, :NW], out["info"][:, :NWH]
        return out

    def run_rows(self, W, nuw, start, tol, max_iter, rows=None, nu_rows=None, want_cov=True):
        """One `vc_gene_kinetics_weighted` call per chunk over the rows of the weight table (rows: a device int64 index into it, gathered
        into a compact table; None: all of them, A = their number).  nuw: host float64 [NW] shared by the rows, or [A, NW] one per row;
        start: None, device float64 [Ng, 2] shared, or [A, Ng, 2]; nu_rows: None (the problem's cycle) or device float64 [A, Ng, K].
        Returns `run`'s device tensors with a leading row axis (cov None when not wanted)."""
        dev, Ng, NW, K = self.dev, self.Ng, int(W.shape[0]), self.K
        NWH = NW * (NW + 1) // 2
        with torch.cuda.device(dev):
            Wt = self.Wt if rows is None else self.Wt[rows].contiguous()
            A = int(Wt.shape[0])
            nuw_d = torch.as_tensor(np.ascontiguousarray(nuw, dtype=np.float64)).to(dev)
            if start is not None:
                start = (torch.as_tensor(start) if not torch.is_tensor(start) else start).to(dev).contiguous()
            if nu_rows is not None:
                nu_rows = nu_rows.contiguous()
            if nuw_d.shape not in ((NW,), (A, NW)) or (start is not None and tuple(start.shape) not in ((Ng, 2), (A, Ng, 2))) or \
                    (nu_rows is not None and tuple(nu_rows.shape) != (A, Ng, K)):
                raise ValueError("the per-row inputs do not match the rows of weights")
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)         # noqa: E731
            i32 = lambda n: torch.empty((A, n), dtype=torch.int32, device=dev)       # noqa: E731
            new = lambda n: dict(xy=f64(A, n, 2), cov=f64(A, n, 3) if want_cov else None, ll=f64(A, n), dec=f64(A, n), it=i32(n),     # noqa: E731
                                 st=i32(n), nc=i32(n), score=f64(A, n, max(NW, 1)), info=f64(A, n, max(NWH, 1)))
            out = new(Ng)
            at = lambda t, off: C.c_void_p(t.data_ptr() + 8 * off)                   # noqa: E731
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for g0, g1, kblk, kind in self.chunks:
                n = g1 - g0
                o = out if n == Ng else new(n)                                       # row b, gene g of a call sits at b * n + g
                sl = lambda t: _ptr(t[g0:g1]) if t is not None else None             # noqa: E731
                nu_p, nu_s = (sl(self.nu), 0) if nu_rows is None else (at(nu_rows, g0 * K), Ng * K)
                st_p, st_s = (None, 0) if start is None else ((sl(start), 0) if start.ndim == 2 else (at(start, g0 * 2), Ng * 2))
                rc = self.lib.vc_gene_kinetics_weighted(_ptr(kblk), kind, n, self.Nc, self.Nc, _ptr(self.B), K, _ptr(self.logm), nu_p, nu_s,
                                                        _ptr(W) if NW else None, NW, _ptr(nuw_d) if NW else None,
                                                        NW if nuw_d.ndim == 2 else 0, self.noise, sl(self.r), sl(self.prior), _ptr(Wt), A,
                                                        self.Nc, st_p, st_s, float(tol), int(max_iter), _ptr(o["xy"]), _ptr(o["cov"]),
                                                        _ptr(o["ll"]), _ptr(o["dec"]), _ptr(o["it"]), _ptr(o["st"]), _ptr(o["nc"]),
                                                        _ptr(o["score"]) if NW else None, _ptr(o["info"]) if NW else None, stream)
                if rc != _lib.VC_OK:
                    raise self.Error(f"vc_gene_kinetics_weighted failed ({rc}): {self.lib.vc_last_error(None).decode()}")
                if o is not out:
                    for key, t in o.items():
                        if t is not None:
                            out[key][:, g0:g1] = t
            torch.cuda.current_stream(dev).synchronize()                             # the gathered table and the slices outlive their launches
            out["score"], out["info"] = out["score"][:, :, :NW], out["info"][:, :, :NWH]
        return out

    def penalty(self, xy):
        """The genes' Gaussian penalties at xy [..., Ng, 2], device float64 [..., Ng]."""
        p = self.prior
        return 0.5 * ((xy[..., 0] - p[:, 0]) / p[:, 1]) ** 2 + 0.5 * ((xy[..., 1] - p[:, 2]) / p[:, 3]) ** 2

    def fit_rows(self, out, squeeze=False):
        """The `GeneKineticsFit` of `run_rows`' tensors: every array with the leading row axis (squeeze: of the one row, without it)."""
        fits = [self.fit({k: t[b] for k, t in out.items()}, self.const[b]) for b in range(out["xy"].shape[0])]
        if squeeze:
            return fits[0]
        return GeneKineticsFit(**{f: np.stack([getattr(x, f) for x in fits]) for f in GeneKineticsFit.__dataclass_fields__})

    def fit(self, out, const=None):
        const = self.const if const is None else const
        NW = out["score"].shape[1]
        info = _unpack_tri(out["info"], NW)
        c = out["cov"]
        cov = torch.stack([torch.stack([c[:, 0], c[:, 1]], 1), torch.stack([c[:, 1], c[:, 2]], 1)], 1)
        return GeneKineticsFit(log_gamma=out["xy"][:, 0].cpu().numpy().copy(), log_beta=out["xy"][:, 1].cpu().numpy().copy(),
                               cov=cov.cpu().numpy(), stds=torch.sqrt(torch.stack([c[:, 0], c[:, 2]])).cpu().numpy(),
                               loglik=(out["ll"] + const).cpu().numpy(), decrement=out["dec"].cpu().numpy(),
                               iterations=out["it"].cpu().numpy(), status=out["st"].cpu().numpy(), n_clamped=out["nc"].cpu().numpy(),
                               score_w=out["score"].cpu().numpy().copy(), info_w=info.cpu().numpy())


def gene_kinetics(counts_U, directions, n_scounts, means, omega=None, a=1, noisemodel="Poisson", dispersion=0.3, *, prior=DEFAULT_PRIOR,
                  start=None, evaluate_only=False, tol=1e-10, max_iter=25, device=None, chunk_genes=None, storage="auto", nu_omega=None,
                  harmonics_w=0, condition_design=None, cell_weights=None, means_replicates=None):
    """(log gamma, log beta) of every gene at the angular speed `omega` (a scalar or one value per cell), on the HIP kernel
    `vc_gene_kinetics`: the maximum over both of the unspliced counts' log-likelihood under the model's Normal priors
    `prior = (mu_gamma, sd_gamma, mu_beta, sd_beta)` (scalars or one value per gene).  counts_U: [Nc, Ng] like an AnnData layer (numpy,
    scipy sparse or torch); directions, n_scounts, a, dispersion, device, chunk_genes, storage: as for `gene_harmonics` (same staging,
    chunking and truncation); means: [2H+1, Ng] like `Cycle.means`, H in {1, 2}.  start: [2, Ng] (rows log gamma, log beta) the
    iteration starts from; evaluate_only=True makes one pass at `start`.  A gene without a count, or with a coefficient that is not
    finite, comes back NO_DATA with NaN outputs.  Returns a `GeneKineticsFit`; its score_w / info_w are those of a common factor on
    omega (the design's one row is omega itself).  With omega=None the speed is that of the coefficients `nu_omega` (condition-major,
    [Nx (2 Hω + 1)]) on the design of `harmonics_w` and `condition_design` (`omega_design`), and score_w / info_w are theirs.

    cell_weights: None (today's path through `vc_gene_kinetics`), or case weights, finite and >= 0, that every cell's contribution is
    multiplied by (`vc_gene_kinetics_weighted`): [Nc], or [R, Nc] for R fits in one call, each array of the result then with a leading
    row axis.  A row that leaves a gene without a weighted count ends NO_DATA there.  means_replicates: [R, 2H+1, Ng] with
    cell_weights [R, Nc]: row b is solved at its own cycle (a jointly resampled one, `GeneHarmonicBootstrap.replicates`)."""
    basis, logm, nu, r, pr, st = check_arguments(counts_U, directions, n_scounts, means, a, noisemodel, dispersion, prior, start,
                                                 evaluate_only, tol, max_iter)
    Wt, nu_rep = check_row_inputs(cell_weights, means_replicates, int(counts_U.shape[0]), nu.shape)
    if (omega is None) == (nu_omega is None):
        raise ValueError("give either omega (per cell) or nu_omega (coefficients on the design of harmonics_w and condition_design)")
    if omega is not None:
        W64, nuw = _check_omega(omega, int(counts_U.shape[0]))[None, :], np.ones(1)
    else:
        W64 = omega_design(directions, harmonics_w, condition_design)
        nuw = np.asarray(nu_omega, dtype=np.float64).reshape(-1)
        if nuw.shape != (W64.shape[0],) or not np.isfinite(nuw).all():
            raise ValueError(f"nu_omega must be {W64.shape[0]} finite coefficients (condition-major)")
    _check_run_options(storage, chunk_genes)
    prob = _Problem(counts_U, basis, logm, nu, r, pr, noisemodel, device, chunk_genes, storage, weights=Wt)
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        if Wt is None:
            return prob.fit(prob.run(W, nuw, st, tol, 0 if evaluate_only else max_iter))
        nu_rows = torch.as_tensor(nu_rep).to(prob.dev) if nu_rep is not None else None
        return prob.fit_rows(prob.run_rows(W, nuw, st, tol, 0 if evaluate_only else max_iter, nu_rows=nu_rows),
                             squeeze=np.ndim(cell_weights) == 1)


def check_row_inputs(cell_weights, means_replicates, Nc, nu_shape):
    """The case weights as `check_weights`' float32 host table [R, Nc] (None: none; a vector is one row) and the per-row cycles
    [R, K, Ng] as float64 [R, Ng, K] (None: none), refused where they do not match."""
    if cell_weights is None:
        if means_replicates is not None:
            raise ValueError("means_replicates needs cell_weights [R, Nc]: one row of case weights per replicate of the cycle")
        return None, None
    w = cell_weights.detach().cpu() if torch.is_tensor(cell_weights) else cell_weights
    Wt = check_weights(w, Nc, rows=1 if np.ndim(w) == 1 else None)
    if means_replicates is None:
        return Wt, None
    rep = np.asarray(means_replicates, dtype=np.float64)
    Ng, K = nu_shape
    if rep.shape != (Wt.shape[0], K, Ng):
        raise ValueError(f"means_replicates must be [rows of weights, 2 harmonics + 1, genes] = ({Wt.shape[0]}, {K}, {Ng}), got {rep.shape}")
    return Wt, np.ascontiguousarray(rep.transpose(0, 2, 1))


def omega_design(directions, harmonics_w=0, condition_design=None):
    """W float64 [Nx (2 Hω + 1), Nc]: row x (2 Hω + 1) + h is the indicator of condition x times row h of zeta_omega(phi)
    (utils.torch_fourier_basis at Hω harmonics, formed from the directions).  condition_design: [Nx, Nc] or None (one condition)."""
    xy = np.asarray(directions, dtype=np.float64)
    if int(harmonics_w) != harmonics_w or harmonics_w < 0:
        raise ValueError("the angular speed's harmonics must be an integer >= 0")
    Nc = xy.shape[1]
    D = np.ones((1, Nc)) if condition_design is None else np.asarray(condition_design, dtype=np.float64)
    if D.ndim != 2 or D.shape[1] != Nc or D.shape[0] < 1:
        raise ValueError(f"condition_design must be [conditions, cells] = (Nx, {Nc}), got {D.shape}")
    if not np.isfinite(D).all():
        raise ValueError("condition_design must be finite")
    zeta = fourier_basis_from_directions(xy, int(harmonics_w)).numpy()
    NW = D.shape[0] * zeta.shape[0]
    if NW > MAX_NW:
        raise ValueError(f"{D.shape[0]} conditions x {zeta.shape[0]} rows of zeta_omega = {NW} coefficients of the angular speed; "
                         f"at most {MAX_NW} are instantiated")
    return (D[:, None, :] * zeta[None, :, :]).reshape(NW, Nc)


def _nuw_prior(prior, Nx, Nhw):
    """(means, precisions) float64 [NW], condition-major, from an `AngularSpeed` (or None: its `trivial_prior`)."""
    if prior is None:
        from .containers import AngularSpeed
        prior = AngularSpeed.trivial_prior(list(range(Nx)), harmonics=(Nhw - 1) // 2)
    m, s = np.asarray(prior.means.values, dtype=np.float64), np.asarray(prior.stds.values, dtype=np.float64)
    if m.shape != (Nhw, Nx) or s.shape != (Nhw, Nx):
        raise ValueError(f"the angular speed's prior must be [2 Hω + 1, conditions] = ({Nhw}, {Nx}), got {m.shape}")
    if not (np.isfinite(m).all() and np.isfinite(s).all() and (s > 0).all()):
        raise ValueError("the angular speed's prior needs finite means and finite stds > 0")
    return np.ascontiguousarray(m.T).reshape(-1), 1.0 / np.ascontiguousarray(s.T).reshape(-1) ** 2


def _solve_spd(J, G):
    L = np.linalg.cholesky(J)
    return np.linalg.solve(L.T, np.linalg.solve(L, G))


def velocity_map(counts_U, directions, n_scounts, means, harmonics_w=0, condition_design=None, a=1, noisemodel="Poisson", dispersion=0.3,
                 *, prior=DEFAULT_PRIOR, nuw_prior=None, nuw_start=None, tol=1e-10, max_iter=25, tol_outer=1e-8, max_rounds=30,
                 device=None, chunk_genes=None, storage="auto", cell_weights=None):
    """The MAP angular speed with every gene's kinetics profiled out:  F(νω) = sum_g max f_g(x, y; νω) - sum_i (νω_i - m_i)^2 / 2 s_i^2,
    `nuw_prior` an `AngularSpeed` over the conditions at `harmonics_w` harmonics (None: its `trivial_prior`).  Per round one
    `vc_gene_kinetics` call per chunk, warm-started from the previous (x, y); the genes' values are summed in float64 by halving;
    G = sum score - Λ (νω - m), J = sum info + Λ, step = J^-1 G, dec = G . step <= tol_outer -> CONVERGED.  A trial point is halved
    while F drops by more than its rounding (8 eps32 sum_g |L_g|), at most 10 times (then STALLED); `max_rounds` steps -> MAX_ROUNDS.
    Genes whose first-round status is not CONVERGED or ROUNDING are left out from then on (`n_excluded`); one that fails later ends
    the fit with GENE_FAILED.  Returns a `VelocityMapFit`.  cell_weights: None (today's path), or one case weight per cell [Nc], finite
    and >= 0: the same iteration on `vc_gene_kinetics_weighted` with one row of weights (ones give the unweighted fit bit for bit);
    many rows side by side are `kinetics_bootstrap.velocity_map_bootstrap`."""
    basis, logm, nu, r, pr, _ = check_arguments(counts_U, directions, n_scounts, means, a, noisemodel, dispersion, prior, None, False,
                                                tol, max_iter)
    Wt = check_weights(cell_weights.detach().cpu() if torch.is_tensor(cell_weights) else cell_weights, int(counts_U.shape[0]), rows=1) \
        if cell_weights is not None else None
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
    prob = _Problem(counts_U, basis, logm, nu, r, pr, noisemodel, device, chunk_genes, storage, weights=Wt)
    ok_codes = (_lib.VC_KIN_CONVERGED, _lib.VC_KIN_ROUNDING)
    with torch.cuda.device(prob.dev):
        W = torch.as_tensor(W64).to(torch.float32).to(prob.dev).contiguous()
        zero = torch.zeros((), dtype=torch.float64, device=prob.dev)
        if Wt is None:
            run, const = (lambda v, start: prob.run(W, v, start, tol, max_iter)), prob.const
        else:                                                                        # the one row of the weighted worker, without its axis
            run, const = (lambda v, start: {k: t[0] for k, t in prob.run_rows(W, v, start, tol, max_iter).items()}), prob.const[0]

        def evaluate(v, start, inc):
            o = run(v, start)
            good = (o["st"] == ok_codes[0]) | (o["st"] == ok_codes[1])
            inc = good if inc is None else inc
            f = torch.where(inc, o["ll"] + const - prob.penalty(o["xy"]), zero)
            mag = torch.where(inc, o["ll"].abs(), zero)
            sums = _row_sums(torch.cat([f[None, :], mag[None, :], torch.where(inc[:, None], o["score"], zero).T,
                                        torch.where(inc[:, None], o["info"], zero).T]).contiguous()).cpu().numpy()
            J = np.zeros((NW, NW))
            J[np.tril_indices(NW)] = sums[2 + NW:]
            J = J + np.tril(J, -1).T + np.diag(pp)
            d = v - pm
            return dict(out=o, inc=inc, failed=bool((inc & ~good).any()), F=float(sums[0] - 0.5 * (pp * d * d).sum()),
                        allow=8.0 * EPS32 * float(sums[1]), G=sums[2:2 + NW] - pp * d, J=J)

        cur = evaluate(nuw, None, None)
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
                    trial = evaluate(nuw + t * step, cur["out"]["xy"], inc)
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
        cov = np.linalg.inv(cur["J"])
        table = lambda v: np.ascontiguousarray(v.reshape(Nx, Nhw).T)                 # noqa: E731
        return VelocityMapFit(nu_omega=table(nuw), stds=table(np.sqrt(np.diag(cov))), cov=cov, F=cur["F"], dec=dec, rounds=rounds,
                              status=status, n_excluded=n_excluded, included=inc.cpu().numpy(), kinetics=prob.fit(cur["out"], const))
