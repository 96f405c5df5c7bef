"""Cell bootstrap of the per-gene harmonic fit (`gene_harmonics` / `Cycle.from_phases_mle`) on the HIP kernel `vc_gene_glm_weighted`.

`GeneHarmonicFit.stds` are sqrt(diag(H^-1)) of the assumed noise model: right when that model is, too narrow when a Poisson fit (or a
negative binomial with one dispersion for every gene) meets overdispersed counts.  The model-free answer resamples the cells: replicate b
draws a Poisson(1) integer weight per cell and fits every gene again under those case weights, warm-started from the full-data fit; the
spread of the replicates is the standard error.  All genes share the resample of a replicate, so replicates carry the cross-gene
covariance.  With the caller's own table the same worker runs a cluster bootstrap (one weight per cluster, repeated over its cells),
exponential (Bayesian bootstrap) weights or held-out fits (0 / 1).

`gene_harmonics_batched_bootstrap` is the same for data pooled from several samples (`gene_batch.gene_harmonics_batched` /
`Cycle.from_phases_batch_mle`) on `vc_gene_glm_batch_weighted`: every replicate estimates the harmonics and the per-batch offsets jointly.

The velocity half has its own module: `kinetics_bootstrap.velocity_map_bootstrap` resamples the MAP angular speed with the same draw
(`draw_weights`: the same seed resamples the same cells) on `vc_gene_kinetics_weighted`, and takes this module's `replicates` as a
jointly resampled cycle.

Limits: no weights in the dispersion worker (`dispersion="mle"`, `gene_dispersion`), and no `dispersion="mle"` with batches; no batch
offsets in the weighted kinetics; no stratified resampling with fixed batch sizes (hand over a table); every row makes its own sweeps (one sweep does not serve
all R rows at the shared warm start); the cells are not sharded (one device holds a gene's row and the weight table); no Lognormal
noise.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from .gene_harmonics import (GeneHarmonicFit, MAX_WEIGHT_ROWS, _check_run_options, _chunks, _open_device, _ptr, check_arguments,
                             check_weights, gene_harmonics)

MAX_REPLICATE_BYTES = 1 << 30        # the [R, K, Ng] float64 replicate array
OK_STATUS = (_lib.VC_GLM_CONVERGED, _lib.VC_GLM_ROUNDING)


@dataclass
class GeneHarmonicBootstrap:
    """Host arrays.  replicates: float64 [R, 2H+1, Ng] (rows [1, sin, cos, sin 2, ...] like `GeneHarmonicFit.means`); status, iterations:
    int32 [R, Ng] (`gene_harmonics.STATUS` names the codes); fit: the full-data `GeneHarmonicFit` the replicates were warm-started
    from; weights: the float32 [R, Nc] table when it was asked for, else None.  Every summary is taken over the `ok` replicates of a
    gene (CONVERGED or ROUNDING): a resample that separates a sparse gene says nothing about its coefficients."""
    replicates: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    fit: Optional[GeneHarmonicFit] = None
    weights: Optional[np.ndarray] = None

    @property
    def harmonics(self):
        return (self.replicates.shape[1] - 1) // 2

    @property
    def ok(self):
        """bool [R, Ng]"""
        return np.isin(self.status, OK_STATUS)

    @property
    def n_ok(self):
        return self.ok.sum(0)

    def _masked(self):
        return np.where(self.ok[:, None, :], self.replicates, np.nan)

    @property
    def means(self):
        """[K, Ng]; NaN for a gene without an ok replicate."""
        n = self.n_ok.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.ok[:, None, :], self.replicates, 0.0).sum(0) / n

    @property
    def cov(self):
        """[Ng, K, K], ddof 1; NaN below 2 ok replicates."""
        n = self.n_ok.astype(np.float64)
        d = np.where(self.ok[:, None, :], self.replicates - np.nan_to_num(self.means)[None], 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.einsum("rig,rjg->gij", d, d) / np.where(n >= 2, n - 1.0, np.nan)[:, None, None]

    @property
    def stds(self):
        """[K, Ng], ddof 1; NaN below 2 ok replicates."""
        return np.sqrt(np.einsum("gii->ig", self.cov))

    @property
    def bias(self):
        return self.means - self.fit.means

    def quantile(self, q):
        """[K, Ng] (q a scalar; an array of q goes in front) over the ok replicates."""
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return np.nanquantile(self._masked(), q, axis=0)

    def amplitude(self, h=1):
        """[R, Ng]: hypot(nu_sin_h, nu_cos_h) of every replicate."""
        self._check_h(h)
        return np.hypot(self.replicates[:, 2 * h - 1], self.replicates[:, 2 * h])

    def peak_phase(self, h=1):
        """[R, Ng]: atan2(nu_sin_h, nu_cos_h) / h, the phase at which harmonic h peaks (in (-pi / h, pi / h])."""
        self._check_h(h)
        return np.arctan2(self.replicates[:, 2 * h - 1], self.replicates[:, 2 * h]) / h

    def interval(self, level=0.95, amplitude=None):
        """Percentile interval (low, high) at `level` over the ok replicates: of the coefficients, [K, Ng] each, or with amplitude=h of
        the amplitude of harmonic h, [Ng] each."""
        if not 0 < level < 1:
            raise ValueError("level must be in (0, 1)")
        lo, hi = (1 - level) / 2, (1 + level) / 2
        if amplitude is None:
            return self.quantile(lo), self.quantile(hi)
        amp = np.where(self.ok, self.amplitude(amplitude), np.nan)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return np.nanquantile(amp, lo, axis=0), np.nanquantile(amp, hi, axis=0)

    def peak_phase_std(self, h=1):
        """[Ng]: the circular standard deviation sqrt(-2 ln |mean e^(i theta)|) / h of the peak of harmonic h, theta = h peak_phase, over the
        ok replicates; NaN below 2."""
        theta = h * self.peak_phase(h)
        ok, n = self.ok, self.n_ok.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rbar = np.hypot(np.where(ok, np.cos(theta), 0.0).sum(0), np.where(ok, np.sin(theta), 0.0).sum(0)) / n
            return np.where(n >= 2, np.sqrt(-2.0 * np.log(np.minimum(rbar, 1.0))) / h, np.nan)

    def _check_h(self, h):
        if int(h) != h or not 1 <= h <= self.harmonics:
            raise ValueError(f"harmonic {h} of a fit with {self.harmonics}")


@dataclass
class GeneBatchHarmonicBootstrap(GeneHarmonicBootstrap):
    """`GeneHarmonicBootstrap` of the batch-aware fit (fit: the full-data `GeneBatchHarmonicFit`), with the offsets of every replicate:
    delta_replicates float64 [R, Nb, Ng] in the caller's batch order, like `GeneBatchHarmonicFit.delta_nu`.  Their summaries run over
    each gene's `ok` replicates, as the coefficients' do.  A batch that a resample empties keeps its offset at the prior mean in that
    replicate: the spread of `delta_nu` then includes how often that happens."""
    delta_replicates: Optional[np.ndarray] = None

    @property
    def delta_nu_means(self):
        """[Nb, Ng]; NaN for a gene without an ok replicate."""
        n = self.n_ok.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.ok[:, None, :], self.delta_replicates, 0.0).sum(0) / n

    @property
    def delta_nu_stds(self):
        """[Nb, Ng], ddof 1; NaN below 2 ok replicates."""
        n = self.n_ok.astype(np.float64)
        d = np.where(self.ok[:, None, :], self.delta_replicates - np.nan_to_num(self.delta_nu_means)[None], 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt((d * d).sum(0) / np.where(n >= 2, n - 1.0, np.nan)[None, :])

    @property
    def delta_nu_bias(self):
        return self.delta_nu_means - self.fit.delta_nu

    def delta_nu_interval(self, level=0.95):
        """Percentile interval (low, high) of the offsets at `level` over the ok replicates, [Nb, Ng] each."""
        if not 0 < level < 1:
            raise ValueError("level must be in (0, 1)")
        masked = np.where(self.ok[:, None, :], self.delta_replicates, np.nan)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return np.nanquantile(masked, (1 - level) / 2, axis=0), np.nanquantile(masked, (1 + level) / 2, axis=0)


def draw_weights(n_boot, Nc, seed, dev):
    """float32 [n_boot, Nc] on `dev`: row b, cell c is the Poisson(1) count of `predictive.sample_counts` (`vc_sample_counts`, the exact
    sampler) at eta = 0 under (seed, draw = b, matrix = 0, index = c).  A pure function of (seed, b, c)."""
    from .predictive import sample_counts
    eta = torch.zeros(Nc, dtype=torch.float32, device=dev)
    out = torch.empty((n_boot, Nc), dtype=torch.float32, device=dev)
    for b in range(n_boot):
        out[b] = sample_counts(eta, seed=seed, draw=b).to(torch.float32)
    return out


def gene_harmonics_bootstrap(counts, directions, n_scounts, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *, n_boot=200, seed=0,
                             weights=None, fit=None, prior_means=None, prior_stds=None, tol=1e-10, max_iter=25, device=None,
                             chunk_genes=None, storage="auto", return_weights=False):
    """counts, directions, n_scounts, harmonics, a, noisemodel, dispersion (a number or one per gene), prior_means, prior_stds, tol,
    max_iter, device, chunk_genes, storage: as for `gene_harmonics`.  Returns a `GeneHarmonicBootstrap` of `n_boot` replicates.

    weights=None: replicate b weighs cell c by a Poisson(1) draw of `predictive.sample_counts` at rate 1 (eta = 0), cast to float32.  The
    draw is keyed onto the sampler's (seed, draw, index) as seed = `seed`, draw = b, matrix = 0, index = c: a pure function of
    (seed, b, c) that knows nothing of n_boot, the chunking or the device, so the first 4 rows of an 8-row run are the 4-row run's.
    weights=[R, Nc]: the caller's table instead (finite, >= 0; n_boot is then R).  fit: the full-data `GeneHarmonicFit` whose `means` are
    the first point of every replicate (None: `gene_harmonics` is run first with the same arguments); it is returned as `.fit`.
    A replicate whose weighted counts of a gene are all zero ends UNBOUNDED for that gene and is left out of its summaries.

    Refused: `dispersion="mle"` (`vc_gene_dispersion` knows no weights), n_boot outside 1..65535, a replicate array above 1 GiB.
    Limits: see the module's docstring."""
    if isinstance(dispersion, str):
        raise ValueError("the bootstrap does not support dispersion='mle': vc_gene_dispersion knows no weights; hand over the estimated "
                         "dispersions (fit.dispersion) instead")
    basis, logm, r, pm, pp = check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means, prior_stds,
                                             tol, max_iter)
    _check_run_options(storage, chunk_genes)
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    K = basis.shape[0]
    w_host = None
    if weights is not None:
        w_host = check_weights(weights, Nc)
        R = w_host.shape[0]
    else:
        if int(n_boot) != n_boot or not 1 <= n_boot <= MAX_WEIGHT_ROWS:
            raise ValueError(f"n_boot must be an integer in 1..{MAX_WEIGHT_ROWS}")
        R = int(n_boot)
    if R * K * Ng * 8 > MAX_REPLICATE_BYTES:
        raise ValueError(f"the replicate array [{R}, {K}, {Ng}] float64 exceeds 1 GiB: bootstrap fewer genes or replicates per call")
    if fit is None:
        fit = gene_harmonics(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means=prior_means,
                             prior_stds=prior_stds, tol=tol, max_iter=max_iter, device=device, chunk_genes=chunk_genes, storage=storage)
    elif np.asarray(fit.means).shape != (K, Ng):
        raise ValueError(f"fit.means must be [2 harmonics + 1, genes] = ({K}, {Ng}), got {np.asarray(fit.means).shape}")
    lib, dev, HipEngineError = _open_device(device)
    ptr = _ptr
    with torch.cuda.device(dev):
        B_d = basis.to(torch.float32).to(dev).contiguous()
        logm_d = logm.to(torch.float32).to(dev).contiguous()
        r_d = r.to(torch.float32).to(dev).contiguous() if r is not None else None
        pm_d = pm.to(dev).contiguous() if pm is not None else None
        pp_d = pp.to(dev).contiguous() if pp is not None else None
        start_d = torch.from_numpy(np.ascontiguousarray(np.asarray(fit.means, dtype=np.float64).T)).to(dev)
        W_d = torch.from_numpy(w_host).to(dev) if w_host is not None else draw_weights(R, Nc, seed, dev)
        nu = torch.empty((R, Ng, K), dtype=torch.float64, device=dev)
        iters = torch.empty((R, Ng), dtype=torch.int32, device=dev)
        status = torch.empty((R, Ng), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0, g1, blk, kblk, kind in _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
            n = g1 - g0
            sl = lambda t: t[g0:g1] if t is not None else None                       # noqa: E731
            nu_c = torch.empty((R, n, K), dtype=torch.float64, device=dev)
            ll_c, dec_c = torch.empty((R, n), dtype=torch.float64, device=dev), torch.empty((R, n), dtype=torch.float64, device=dev)
            it_c, st_c = torch.empty((R, n), dtype=torch.int32, device=dev), torch.empty((R, n), dtype=torch.int32, device=dev)
            rc = lib.vc_gene_glm_weighted(ptr(kblk), kind, n, Nc, Nc, ptr(B_d), K, ptr(logm_d), _lib.NOISE[noisemodel], ptr(sl(r_d)),
                                          ptr(sl(pm_d)), ptr(sl(pp_d)), ptr(W_d), R, Nc, ptr(start_d[g0:g1]), float(tol), int(max_iter),
                                          ptr(nu_c), None, ptr(ll_c), ptr(dec_c), ptr(it_c), ptr(st_c), stream)
            if rc != _lib.VC_OK:
                raise HipEngineError(f"vc_gene_glm_weighted failed ({rc}): {lib.vc_last_error(None).decode()}")
            nu[:, g0:g1], iters[:, g0:g1], status[:, g0:g1] = nu_c, it_c, st_c
            torch.cuda.current_stream(dev).synchronize()                             # the block and the chunk's outputs outlive their launch
            del blk, kblk
        return GeneHarmonicBootstrap(replicates=nu.permute(0, 2, 1).contiguous().cpu().numpy(), status=status.cpu().numpy(),
                                     iterations=iters.cpu().numpy(), fit=fit, weights=W_d.cpu().numpy() if return_weights else None)


def gene_harmonics_batched_bootstrap(counts, directions, n_scounts, batches, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *,
                                     n_boot=200, seed=0, weights=None, fit=None, delta_nu_prior=(0.0, 0.5), prior_means=None,
                                     prior_stds=None, tol=1e-10, max_iter=25, device=None, chunk_genes=None, storage="auto",
                                     return_weights=False):
    """The cell bootstrap of `gene_batch.gene_harmonics_batched` on `vc_gene_glm_batch_weighted`: every replicate fits the harmonics and
    the batch offsets again, jointly, under its case weights.  counts, directions, n_scounts, batches, harmonics, a, noisemodel,
    dispersion (a number or one per gene), delta_nu_prior, prior_means, prior_stds, tol, max_iter, device, chunk_genes, storage: as for
    `gene_harmonics_batched`.  Returns a `GeneBatchHarmonicBootstrap` of `n_boot` replicates.

    weights=None: the table is `draw_weights(n_boot, Nc, seed, dev)`: row b, cell c is keyed by (seed, b, c) in the CALLER's cell order,
    so the same seed resamples the same cells as `gene_harmonics_bootstrap`, whatever the batches.  weights=[R, Nc]: the caller's table
    (finite, >= 0; n_boot is then R), e.g. a stratified resample with fixed batch sizes.  Either way the columns are permuted by
    `batch_segments`' permutation together with the basis, the offsets of eta and the staged block; `return_weights` gives the table in
    the caller's order.  fit: the full-data `GeneBatchHarmonicFit` whose `means` and `delta_nu` are the first point of every replicate
    (None: `gene_harmonics_batched` is run first with the same arguments); it is returned as `.fit`.  No covariances are stored.  A
    replicate that empties a batch keeps that offset at its prior mean; one whose weighted counts of a gene are all zero ends UNBOUNDED
    for that gene and is left out of its summaries.

    Refused: `dispersion` as a string (`vc_gene_dispersion` knows neither offsets nor weights), n_boot outside 1..65535, replicate arrays
    ([R, K, Ng] and [R, Nb, Ng] float64) above 1 GiB together."""
    from .gene_batch import batch_labels, batch_segments, delta_prior, gene_harmonics_batched
    if isinstance(dispersion, str):
        raise ValueError(f"the batch bootstrap does not support dispersion={dispersion!r}: vc_gene_dispersion knows neither the batch "
                         "offsets nor weights; pass a number or one number per gene")
    basis, logm, r, pm, pp = check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means, prior_stds,
                                             tol, max_iter)
    _check_run_options(storage, chunk_genes)
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    K = basis.shape[0]
    labels, Nb = batch_labels(batches, Nc)
    dm, dq = delta_prior(delta_nu_prior, Nb, Ng)
    w_host = None
    if weights is not None:
        w_host = check_weights(weights, Nc)
        R = w_host.shape[0]
    else:
        if int(n_boot) != n_boot or not 1 <= n_boot <= MAX_WEIGHT_ROWS:
            raise ValueError(f"n_boot must be an integer in 1..{MAX_WEIGHT_ROWS}")
        R = int(n_boot)
    if R * (K + Nb) * Ng * 8 > MAX_REPLICATE_BYTES:
        raise ValueError(f"the replicate arrays [{R}, {K}, {Ng}] and [{R}, {Nb}, {Ng}] float64 exceed 1 GiB together: bootstrap fewer genes "
                         "or replicates per call")
    if fit is None:
        fit = gene_harmonics_batched(counts, directions, n_scounts, batches, harmonics, a, noisemodel, dispersion,
                                     delta_nu_prior=delta_nu_prior, prior_means=prior_means, prior_stds=prior_stds, tol=tol,
                                     max_iter=max_iter, device=device, chunk_genes=chunk_genes, storage=storage)
    elif np.asarray(fit.means).shape != (K, Ng) or np.asarray(fit.delta_nu).shape != (Nb, Ng):
        raise ValueError(f"fit.means must be [2 harmonics + 1, genes] = ({K}, {Ng}) and fit.delta_nu [batches, genes] = ({Nb}, {Ng}), got "
                         f"{np.asarray(fit.means).shape} and {np.asarray(fit.delta_nu).shape}")
    perm, seg = batch_segments(labels, Nb)
    seg = (C.c_int64 * (Nb + 1))(*seg)
    lib, dev, HipEngineError = _open_device(device)
    ptr = _ptr
    with torch.cuda.device(dev):
        perm_d = torch.from_numpy(perm).to(dev)
        B_d = basis[:, perm].to(torch.float32).to(dev).contiguous()
        logm_d = logm[perm].to(torch.float32).to(dev).contiguous()
        r_d = r.to(torch.float32).to(dev).contiguous() if r is not None else None
        pm_d = pm.to(dev).contiguous() if pm is not None else None
        pp_d = pp.to(dev).contiguous() if pp is not None else None
        dm_d, dq_d = dm.to(dev).contiguous(), dq.to(dev).contiguous()
        start_nu = torch.from_numpy(np.ascontiguousarray(np.asarray(fit.means, dtype=np.float64).T)).to(dev)
        start_delta = torch.from_numpy(np.ascontiguousarray(np.asarray(fit.delta_nu, dtype=np.float64).T)).to(dev)
        W_d = torch.from_numpy(w_host).to(dev) if w_host is not None else draw_weights(R, Nc, seed, dev)   # the caller's cell order
        Wp_d = W_d[:, perm_d].contiguous()                                           # sorted like the cells the kernel reads
        nu = torch.empty((R, Ng, K), dtype=torch.float64, device=dev)
        delta = torch.empty((R, Ng, Nb), dtype=torch.float64, device=dev)
        iters = torch.empty((R, Ng), dtype=torch.int32, device=dev)
        status = torch.empty((R, Ng), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0, g1, blk, kblk, kind in _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
            n = g1 - g0
            sl = lambda t: t[g0:g1] if t is not None else None                       # noqa: E731
            kblk = kblk[:, perm_d].contiguous()                                      # cells of a batch contiguous, batches in order
            nu_c = torch.empty((R, n, K), dtype=torch.float64, device=dev)
            dl_c = torch.empty((R, n, Nb), dtype=torch.float64, device=dev)
            ll_c, dec_c = torch.empty((R, n), dtype=torch.float64, device=dev), torch.empty((R, n), dtype=torch.float64, device=dev)
            it_c, st_c = torch.empty((R, n), dtype=torch.int32, device=dev), torch.empty((R, n), dtype=torch.int32, device=dev)
            rc = lib.vc_gene_glm_batch_weighted(ptr(kblk), kind, n, Nc, Nc, ptr(B_d), K, ptr(logm_d), _lib.NOISE[noisemodel], ptr(sl(r_d)),
                                                Nb, seg, ptr(dm_d[g0:g1]), ptr(dq_d[g0:g1]), ptr(sl(pm_d)), ptr(sl(pp_d)), ptr(Wp_d), R, Nc,
                                                ptr(start_nu[g0:g1]), ptr(start_delta[g0:g1]), float(tol), int(max_iter), ptr(nu_c),
                                                ptr(dl_c), None, None, ptr(ll_c), ptr(dec_c), ptr(it_c), ptr(st_c), stream)
            if rc != _lib.VC_OK:
                raise HipEngineError(f"vc_gene_glm_batch_weighted failed ({rc}): {lib.vc_last_error(None).decode()}")
            nu[:, g0:g1], delta[:, g0:g1], iters[:, g0:g1], status[:, g0:g1] = nu_c, dl_c, it_c, st_c
            torch.cuda.current_stream(dev).synchronize()                             # the block and the chunk's outputs outlive their launch
            del blk, kblk
        return GeneBatchHarmonicBootstrap(replicates=nu.permute(0, 2, 1).contiguous().cpu().numpy(), status=status.cpu().numpy(),
                                          iterations=iters.cpu().numpy(), fit=fit, weights=W_d.cpu().numpy() if return_weights else None,
                                          delta_replicates=delta.permute(0, 2, 1).contiguous().cpu().numpy())
