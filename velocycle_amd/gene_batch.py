"""Batch-aware per-gene harmonic regression given the cells' phases (the worker behind `Cycle.from_phases_batch_mle`) on the HIP
kernel `vc_gene_glm_batch`.

The model is `gene_harmonics`' with the phase model's per-batch offsets (phase_inference_model: ElogS = nu . zeta(phi) + Db . dnu +
count_factor, dnu[b, g] ~ Normal(mu_dnu, sigma_dnu)):

    mu_gc = exp(nu_g . zeta(phi_c) + dnu[b(c), g]) * n_c^a

For every gene the kernel maximises the log-likelihood minus the Gaussian penalty of the offsets (always there: it is what tells nu_0
from the mean of the offsets) and, optionally, of nu, jointly over nu and dnu by a damped Newton iteration.  The null model of the
likelihood-ratio statistic is the same kernel at K = 1 -- a constant plus the batch offsets -- so `lr_stat` tests periodicity GIVEN the
batches.

The cells are sorted by batch (a stable permutation of the basis, the offsets of eta and the staged block); staging, chunking and the
lgamma constants are `gene_harmonics`' own.  The result does not depend on `chunk_genes`, uint16 / float32 storage, dense / CSR input or
repetition bit for bit, and on the order of the cells only through the order of the sums.  `dispersion="mle"` is refused:
`vc_gene_dispersion` does not know the offsets.  With `cell_weights=` the same fit runs under one row of case weights on
`vc_gene_glm_batch_weighted`; `gene_bootstrap.gene_harmonics_batched_bootstrap` solves many rows per call.  There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .gene_harmonics import (GeneHarmonicFit, _check_run_options, _chunks, _constants, _open_device, _ptr, _unpack_tri, check_arguments,
                             check_weights)

MAX_BATCHES = _lib.VC_GLM_MAX_BATCHES


@dataclass
class GeneBatchHarmonicFit:
    """Host float64 arrays.  The fields of `GeneHarmonicFit` (cov: the nu block of the inverse Hessian, [Ng, 2H+1, 2H+1]; loglik_null:
    the fit of a constant plus the batch offsets), and delta_nu, delta_nu_stds: [Nb, Ng], the offsets and the square roots of the
    diagonal of the delta block of the inverse Hessian, in the caller's batch order (the column order of the one-hot design, or the
    label values 0..Nb-1)."""
    means: np.ndarray
    stds: np.ndarray
    cov: np.ndarray
    loglik: np.ndarray
    loglik_null: np.ndarray
    decrement: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    delta_nu: np.ndarray
    delta_nu_stds: np.ndarray

    bootstrap = None                 # not a field: `Cycle.from_phases_batch_mle(bootstrap=n)` hangs its GeneBatchHarmonicBootstrap here

    harmonics = GeneHarmonicFit.harmonics
    lr_stat = GeneHarmonicFit.lr_stat
    dof = GeneHarmonicFit.dof
    p_value = GeneHarmonicFit.p_value


def batch_labels(batches, Nc):
    """A one-hot [Nc, Nb] design (as `make_design_matrix` returns) or an integer label vector [Nc] -> (int64 labels [Nc], Nb).
    Refused by name: a design that is not one-hot, a batch without a cell, more than VC_GLM_MAX_BATCHES batches."""
    b = batches.detach().cpu().numpy() if torch.is_tensor(batches) else np.asarray(batches)
    if b.ndim == 2:
        if b.shape[0] != Nc or b.shape[1] < 1:
            raise ValueError(f"the batch design must be [cells, batches] = ({Nc}, Nb), got {b.shape}")
        if not (((b == 0) | (b == 1)).all() and (b.sum(1) == 1).all()):
            raise ValueError("the batch design is not one-hot: every cell needs exactly one 1 (designs that are not one-hot are not implemented)")
        Nb = b.shape[1]
        labels = np.argmax(b, axis=1).astype(np.int64)
    elif b.ndim == 1:
        if b.shape[0] != Nc:
            raise ValueError(f"the batch labels have {b.shape[0]} entries for {Nc} cells")
        if b.dtype.kind not in "iub" and not (np.isfinite(b).all() and (b == np.trunc(b)).all()):
            raise ValueError("the batch labels must be integers 0..Nb-1 (or pass a one-hot design)")
        labels = b.astype(np.int64)
        if labels.min() < 0:
            raise ValueError("the batch labels must be integers 0..Nb-1 (or pass a one-hot design)")
        Nb = int(labels.max()) + 1
    else:
        raise ValueError("batches must be a one-hot [cells, batches] design or an integer label vector [cells]")
    if Nb > MAX_BATCHES:
        raise ValueError(f"{Nb} batches: vc_gene_glm_batch takes at most VC_GLM_MAX_BATCHES = {MAX_BATCHES}")
    sizes = np.bincount(labels, minlength=Nb)
    if (sizes == 0).any():
        raise ValueError(f"batch {int(np.flatnonzero(sizes == 0)[0])} has no cell: an empty batch has no offset to estimate")
    return labels, Nb


def delta_prior(delta_nu_prior, Nb, Ng):
    """(mean, std), scalars or [Nb, Ng] -> (means, precisions) float64 [Ng, Nb] tensors.  The std must be finite and > 0."""
    if delta_nu_prior is None or len(delta_nu_prior) != 2:
        raise ValueError("delta_nu_prior is (mean, std) of the batch offsets; every offset needs its prior")
    out = []
    for v in delta_nu_prior:
        v = np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
        if v.ndim not in (0, 2) or (v.ndim == 2 and v.shape != (Nb, Ng)):
            raise ValueError(f"delta_nu_prior's mean and std must be scalars or [batches, genes] = ({Nb}, {Ng}), got {v.shape}")
        out.append(np.broadcast_to(v, (Nb, Ng)))
    mean, std = out
    if not np.isfinite(mean).all():
        raise ValueError("delta_nu_prior's mean must be finite")
    if not (np.isfinite(std).all() and (std > 0).all()):
        raise ValueError("delta_nu_prior's std must be finite and > 0")
    return torch.as_tensor(np.ascontiguousarray(mean.T)), torch.as_tensor(np.ascontiguousarray(1.0 / std.T ** 2))


def batch_segments(labels, Nb):
    """(perm, seg): the stable permutation that makes the cells of a batch contiguous, batches in order, and the Nb + 1 segment bounds
    (batch b owns the sorted cells [seg[b], seg[b + 1]))."""
    return np.argsort(labels, kind="stable"), [0, *np.cumsum(np.bincount(labels, minlength=Nb)).tolist()]


def gene_harmonics_batched(counts, directions, n_scounts, batches, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *,
                           delta_nu_prior=(0.0, 0.5), prior_means=None, prior_stds=None, tol=1e-10, max_iter=25, device=None,
                           chunk_genes=None, storage="auto", **options):
    """counts, directions, n_scounts, harmonics, a, noisemodel, prior_means / prior_stds, tol, max_iter, device, chunk_genes, storage: as
    for `gene_harmonics`.  batches: a one-hot [Nc, Nb] design as `make_design_matrix` returns, or an integer label vector [Nc].
    delta_nu_prior: (mean, std) of the offsets, scalars or [Nb, Ng]; the defaults are the phase model's.  dispersion: a scalar or [Ng]
    ("mle" is refused).  Returns a `GeneBatchHarmonicFit`.

    cell_weights (accepted by name only, default None): [Nc] finite case weights >= 0 in the caller's cell order (float32 on the device).
    Every cell's term of the log-likelihood, of its gradient and of its Hessian is multiplied by its weight, in the fit and in the null
    model (K = 1 with offsets) alike, on `vc_gene_glm_batch_weighted` (one row, default start); the priors are not weighted; `loglik` and
    `loglik_null` carry the weighted constants as `gene_harmonics`' do.  A vector of ones returns the unweighted result bit for bit.  A
    batch whose cells all weigh 0 keeps its offset at the prior mean."""
    cell_weights = options.pop("cell_weights", None)                                 # by name only: the signature is pinned
    if options:
        raise TypeError(f"gene_harmonics_batched() got unexpected keyword arguments {sorted(options)}")
    if isinstance(dispersion, str):
        if dispersion == "mle":
            raise ValueError("dispersion='mle' is not available with batches: vc_gene_dispersion does not know the batch offsets yet; "
                             "pass a number or one number per gene")
        raise ValueError(f"dispersion must be a number or one number per gene, got {dispersion!r}")
    basis, logm, r, pm, pp = check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means, prior_stds,
                                             tol, max_iter)
    _check_run_options(storage, chunk_genes)
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    w_host = check_weights(cell_weights, Nc, rows=1) if cell_weights is not None else None
    labels, Nb = batch_labels(batches, Nc)
    dm, dq = delta_prior(delta_nu_prior, Nb, Ng)
    perm, seg = batch_segments(labels, Nb)
    seg = (C.c_int64 * (Nb + 1))(*seg)
    lib, dev, HipEngineError = _open_device(device)
    K = basis.shape[0]
    NH = K * (K + 1) // 2
    ptr = _ptr
    with torch.cuda.device(dev):
        perm_d = torch.from_numpy(perm).to(dev)
        w_d = torch.from_numpy(w_host[:, perm]).to(dev).contiguous() if w_host is not None else None   # sorted like the cells
        w64 = w_d[0].double() if w_d is not None else None
        B_d = basis[:, perm].to(torch.float32).to(dev).contiguous()
        logm_d = logm[perm].to(torch.float32).to(dev).contiguous()
        r_d = r.to(torch.float32).to(dev).contiguous() if r is not None else None
        r64 = r_d.double() if r_d is not None else None                          # the model is the one of the float32 r the kernel reads
        pm_d = pm.to(dev).contiguous() if pm is not None else None
        pp_d = pp.to(dev).contiguous() if pp is not None else None
        dm_d, dq_d = dm.to(dev).contiguous(), dq.to(dev).contiguous()
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)  # noqa: E731
        i32 = lambda: torch.empty(Ng, dtype=torch.int32, device=dev)             # noqa: E731
        full = dict(nu=f64(Ng, K), delta=f64(Ng, Nb), cov=f64(Ng, NH), dvar=f64(Ng, Nb), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32())
        null = dict(nu=f64(Ng, 1), delta=f64(Ng, Nb), cov=f64(Ng, 1), dvar=f64(Ng, Nb), ll=f64(Ng), dec=f64(Ng), it=i32(), st=i32())
        const = f64(Ng)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0, g1, blk, kblk, kind in _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
            same = kblk is blk
            blk = blk[:, perm_d].contiguous()                                        # cells of a batch contiguous, batches in order
            kblk = blk if same else kblk[:, perm_d].contiguous()
            const[g0:g1] = _constants(blk, r64[g0:g1] if r64 is not None else None, w64)
            # the fit, then the constant with the offsets (K = 1: the null model, under the prior's nu0 column)
            for k_, outs, pm_c, pp_c in ((K, full, pm_d[g0:g1] if pm_d is not None else None, pp_d[g0:g1] if pp_d is not None else None),
                                         (1, null, pm_d[g0:g1, :1].contiguous() if pm_d is not None else None,
                                          pp_d[g0:g1, :1].contiguous() if pp_d is not None else None)):
                head = (ptr(kblk), kind, g1 - g0, Nc, Nc, ptr(B_d), k_, ptr(logm_d), _lib.NOISE[noisemodel],
                        ptr(r_d[g0:g1]) if r_d is not None else None, Nb, seg, ptr(dm_d[g0:g1]), ptr(dq_d[g0:g1]), ptr(pm_c), ptr(pp_c))
                tail = (float(tol), int(max_iter), *[ptr(outs[n][g0:g1]) for n in ("nu", "delta", "cov", "dvar", "ll", "dec", "it", "st")], stream)
                if w_d is not None:                                              # one row of case weights, each gene from its default start
                    fn, rc = "vc_gene_glm_batch_weighted", lib.vc_gene_glm_batch_weighted(*head, ptr(w_d), 1, Nc, None, None, *tail)
                else:
                    fn, rc = "vc_gene_glm_batch", lib.vc_gene_glm_batch(*head, *tail)
                if rc != _lib.VC_OK:
                    raise HipEngineError(f"{fn} failed ({rc}): {lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # the block and the slices outlive their launches
            del blk, kblk
        cov = _unpack_tri(full["cov"], K)
        stds = torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2))
        return GeneBatchHarmonicFit(means=full["nu"].T.cpu().numpy().copy(), stds=stds.T.cpu().numpy().copy(), cov=cov.cpu().numpy(),
                                    loglik=(full["ll"] + const).cpu().numpy(), loglik_null=(null["ll"] + const).cpu().numpy(),
                                    decrement=full["dec"].cpu().numpy(), iterations=full["it"].cpu().numpy(),
                                    status=full["st"].cpu().numpy(), delta_nu=full["delta"].T.cpu().numpy().copy(),
                                    delta_nu_stds=torch.sqrt(full["dvar"]).T.cpu().numpy().copy())
