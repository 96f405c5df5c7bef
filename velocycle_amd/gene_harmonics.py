"""Per-gene harmonic regression given the cells' phases (the worker behind `Cycle.from_phases_mle`) on the HIP kernel `vc_gene_glm`.

The model is the one of `Phases.from_cycle_mle` (reference velocycle/phases.py:487-507), solved for the other factor:

    mu_gc = exp(nu_g . zeta(phi_c)) * n_c^a,   zeta = [1, sin phi, cos phi, sin 2 phi, ...]   (utils.torch_fourier_basis)
    Poisson            log p = k eta - mu - lgamma(k + 1)
    NegativeBinomial   log p = lgamma(k + r) - lgamma(r) - lgamma(k + 1) + r log r + k eta - (k + r) log(r + mu),   r = 1 / dispersion

For every gene the kernel maximises the log-likelihood over nu (optionally minus a Gaussian penalty per coefficient) by a damped Newton
iteration and returns nu, the inverse observed Hessian, the nu-dependent log-likelihood and how the iteration ended.  A second pass
with the constant alone gives the null model of the likelihood-ratio statistic for periodicity.

Genes are independent: they are walked in chunks, each chunk a dense [genes][cells] device block (a sparse layer is scattered into it
on the device), and the result does not depend on the chunk size bit for bit.  Cells cannot be cut.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .phase_mle import CHUNK_BYTES, NOISEMODELS, _is_sparse

MAX_HARMONICS = 3                    # csrc/vc_gene_glm.hip
STATUS = {_lib.VC_GLM_CONVERGED: "CONVERGED", _lib.VC_GLM_ROUNDING: "ROUNDING", _lib.VC_GLM_UNBOUNDED: "UNBOUNDED",
          _lib.VC_GLM_SINGULAR: "SINGULAR", _lib.VC_GLM_MAX_ITER: "MAX_ITER"}


@dataclass
class GeneHarmonicFit:
    """Host float64 arrays.  means, stds: [2H+1, Ng] (rows [1, sin, cos, sin 2, ...], the layout of `Cycle.means`); cov: [Ng, 2H+1, 2H+1]
    (the inverse observed Hessian; stds = sqrt of its diagonal); loglik, loglik_null: [Ng] full log-likelihoods at the fit and at the
    fit of the constant alone; decrement: the last Newton decrement; iterations, status: int32 [Ng] (`STATUS` names the codes)."""
    means: np.ndarray
    stds: np.ndarray
    cov: np.ndarray
    loglik: np.ndarray
    loglik_null: np.ndarray
    decrement: np.ndarray
    iterations: np.ndarray
    status: np.ndarray

    @property
    def harmonics(self):
        return (self.means.shape[0] - 1) // 2

    @property
    def lr_stat(self):
        return 2.0 * (self.loglik - self.loglik_null)

    @property
    def dof(self):
        return 2 * self.harmonics

    @property
    def p_value(self):
        """Chi-square survival function of lr_stat at dof = 2H, float64 on the host.  The degrees of freedom are even, so it is the
        finite sum  exp(-x / 2) sum_{j < H} (x / 2)^j / j!;  H = 0 has nothing to test: 1."""
        x = np.maximum(np.asarray(self.lr_stat, dtype=np.float64), 0.0) / 2.0
        s = np.zeros_like(x)
        for j in range(self.harmonics):
            s += x ** j / math.factorial(j)
        return np.where(np.isnan(self.lr_stat), np.nan, np.exp(-x) * s) if self.harmonics else np.ones_like(x)


def default_chunk_genes(Nc: int) -> int:
    """Genes per chunk such that the chunk's dense float32 block stays within CHUNK_BYTES (at least 1)."""
    return max(1, CHUNK_BYTES // (4 * int(Nc)))


def fourier_basis_from_directions(directions, harmonics):
    """[2H+1, Nc] float64 rows [1, sin phi, cos phi, sin 2 phi, ...] from the phase directions (x, y) = |xy| (cos phi, sin phi), by
    angle addition: no angle is ever formed, so none is rounded."""
    xy = torch.as_tensor(np.asarray(directions, dtype=np.float64))
    norm = torch.sqrt(xy[0] ** 2 + xy[1] ** 2)
    c1, s1 = xy[0] / norm, xy[1] / norm
    rows, c, s = [torch.ones_like(c1)], torch.ones_like(c1), torch.zeros_like(c1)
    for _ in range(harmonics):
        c, s = c * c1 - s * s1, s * c1 + c * s1
        rows += [s, c]
    return torch.stack(rows)


def gene_totals(counts):
    """Sum per gene of the counts truncated to integers, float64 on the host for host inputs."""
    if _is_sparse(counts):
        coo = counts.tocoo(copy=True)
        coo.sum_duplicates()
        return np.bincount(coo.col, weights=np.trunc(np.asarray(coo.data, dtype=np.float64)), minlength=counts.shape[1])
    if torch.is_tensor(counts):
        return counts.detach().to(torch.float64).trunc().sum(0).cpu().numpy()
    counts = np.asarray(counts)
    tot = np.zeros(counts.shape[1], dtype=np.float64)
    for i in range(0, counts.shape[0], 4096):                       # in blocks of cells: no float64 copy of the whole matrix
        tot += np.trunc(counts[i:i + 4096]).sum(0, dtype=np.float64)
    return tot


def check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means=None, prior_stds=None,
                    tol=1e-10, max_iter=25):
    """Every refusal that needs no device.  Returns (basis float64 [K, Nc], logm float64 [Nc], r float64 [Ng] or None,
    prior means float64 [Ng, K] or None, prior precisions float64 [Ng, K] or None)."""
    if noisemodel not in NOISEMODELS:
        raise NotImplementedError("Not implemented yet, sorry")
    if int(harmonics) != harmonics or not 0 <= harmonics <= MAX_HARMONICS:
        raise ValueError(f"harmonics must be an integer in 0..{MAX_HARMONICS}")
    harmonics = int(harmonics)
    K = 2 * harmonics + 1
    if len(counts.shape) != 2 or counts.shape[0] < 1 or counts.shape[1] < 1:
        raise ValueError("counts must be [cells, genes] with at least one of each")
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    xy = np.asarray(directions, dtype=np.float64)
    if xy.shape != (2, Nc):
        raise ValueError(f"directions must be [2, cells] = (2, {Nc}) like Phases.phi_xy, got {xy.shape}")
    norm2 = xy[0] ** 2 + xy[1] ** 2
    if not (np.isfinite(norm2).all() and (norm2 > 0).all()):
        raise ValueError("every cell needs a finite phase direction of non-zero length")
    n = np.asarray(n_scounts, dtype=np.float64).reshape(-1)
    if n.size != Nc:
        raise ValueError(f"n_scounts has {n.size} entries for {Nc} cells")
    if not (np.isfinite(n).all() and (n > 0).all()):
        raise ValueError("every cell needs a finite n_scounts > 0")
    if not (tol >= 0):
        raise ValueError("tol must be >= 0")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("max_iter must be an integer >= 1")
    r = None
    if noisemodel == "NegativeBinomial":
        d = torch.as_tensor(np.asarray(dispersion, dtype=np.float64)).reshape(-1)
        if d.numel() not in (1, Ng):
            raise ValueError(f"dispersion must be a scalar or one value per gene ({Ng}), got {d.numel()}")
        if not bool((torch.isfinite(d) & (d > 0)).all()):
            raise ValueError("dispersion must be > 0")
        r = (1.0 / d).expand(Ng).contiguous()
    if (prior_means is None) != (prior_stds is None):
        raise ValueError("a prior needs both prior_means and prior_stds")
    pm = pp = None
    if prior_means is not None:
        pm = np.asarray(prior_means, dtype=np.float64)
        ps = np.asarray(prior_stds, dtype=np.float64)
        if pm.shape != (K, Ng) or ps.shape != (K, Ng):
            raise ValueError(f"prior_means and prior_stds must be [2 harmonics + 1, genes] = ({K}, {Ng}), got {pm.shape} and {ps.shape}")
        if (ps <= 0).any():
            raise ValueError("prior_stds must be > 0")
        pm = torch.as_tensor(np.ascontiguousarray(pm.T))
        with np.errstate(over="ignore"):
            pp = torch.as_tensor(np.ascontiguousarray(1.0 / ps.T ** 2))
    empty = int((gene_totals(counts) <= 0).sum())
    if empty:
        raise ValueError(f"{empty} of {Ng} genes have no count in any cell: they have no maximum-likelihood fit; filter them out first")
    basis = fourier_basis_from_directions(xy, harmonics)
    logm = float(a) * torch.log(torch.as_tensor(n))
    return basis, logm, r, pm, pp


def _gene_block(counts, g0, g1, Nc, dev):
    """Genes [g0, g1) as a float32 device block [g1 - g0][Nc], truncated to integers like `phase_mle._dense_block`."""
    n = g1 - g0
    if _is_sparse(counts):
        sub = counts[:, g0:g1].tocoo()
        blk = torch.zeros((n, Nc), dtype=torch.float32, device=dev)
        if sub.nnz:
            rows = torch.from_numpy(sub.row.astype(np.int64)).to(dev)
            cols = torch.from_numpy(sub.col.astype(np.int64)).to(dev)
            val = torch.from_numpy(np.asarray(sub.data, dtype=np.float32)).to(dev)
            blk.index_put_((cols, rows), val, accumulate=True)
        return blk.trunc_()
    part = counts[:, g0:g1]
    part = part if torch.is_tensor(part) else torch.from_numpy(np.ascontiguousarray(part))
    return part.to(dev).to(torch.float32).T.clone(memory_format=torch.contiguous_format).trunc_()


def _row_sums(x):
    """[n, L] float64 -> [n]: halving by elementwise additions only, so that a row's bits do not depend on how many rows go with it
    (a library reduction may pick its order by the shape)."""
    while x.shape[1] > 1:
        L = x.shape[1]
        h = (L + 1) // 2
        lo = x[:, :h].clone()
        lo[:, :L - h] += x[:, h:]
        x = lo
    return x[:, 0]


def _constants(blk, r64):
    """The part of every gene's log-likelihood that does not depend on nu and that the kernel leaves out, float64 [n]:
    -lgamma(k + 1), and for the negative binomial lgamma(k + r) - lgamma(r) (its r log r is inside the kernel's objective)."""
    out = torch.empty(blk.shape[0], dtype=torch.float64, device=blk.device)
    rows = max(1, (1 << 24) // blk.shape[1])
    for i in range(0, blk.shape[0], rows):
        k = blk[i:i + rows].double()
        t = -torch.lgamma(k + 1.0)
        if r64 is not None:
            rr = r64[i:i + rows, None]
            t += torch.lgamma(k + rr) - torch.lgamma(rr)
        out[i:i + rows] = _row_sums(t)
    return out


def gene_harmonics(counts, directions, n_scounts, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *, prior_means=None,
                   prior_stds=None, tol=1e-10, max_iter=25, device=None, chunk_genes=None, storage="auto"):
    """counts: [Nc, Ng] cell-major like an AnnData layer (numpy, scipy sparse or torch); directions: [2, Nc] phase directions (rows x, y
    like `Phases.phi_xy`, any length > 0); n_scounts: [Nc] > 0; dispersion: scalar or [Ng]; prior_means / prior_stds: [2H+1, Ng] like
    `Cycle.means` / `Cycle.stds` (a coefficient with a non-finite mean or std has no prior).  storage: "auto" (uint16 per chunk when every
    count is an integer <= 65535) | "f32" | "u16".  Returns a `GeneHarmonicFit`."""
    basis, logm, r, pm, pp = check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel, dispersion, prior_means, prior_stds,
                                             tol, max_iter)
    if storage not in ("auto", "f32", "u16"):
        raise ValueError(f"unknown storage {storage!r}")
    if chunk_genes is not None and int(chunk_genes) < 1:
        raise ValueError("chunk_genes must be >= 1")
    lib = _lib.load()
    from .engine import HipEngineError
    if not torch.cuda.is_available():
        raise HipEngineError("velocycle_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    K = basis.shape[0]
    NH = K * (K + 1) // 2
    if _is_sparse(counts):
        counts = counts.tocsc()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    with torch.cuda.device(dev):
        B_d = basis.to(torch.float32).to(dev).contiguous()
        logm_d = logm.to(torch.float32).to(dev).contiguous()
        r_d = r.to(torch.float32).to(dev).contiguous() if r is not None else None
        r64 = r_d.double() if r_d is not None else None                          # the model is the one of the float32 r the kernel reads
        pm_d = pm.to(dev).contiguous() if pm is not None else None
        pp_d = pp.to(dev).contiguous() if pp is not None else None
        nu = torch.empty((Ng, K), dtype=torch.float64, device=dev)
        cov = torch.empty((Ng, NH), dtype=torch.float64, device=dev)
        out = {n: torch.empty(Ng, dtype=torch.float64, device=dev) for n in ("ll", "dec", "ll0")}
        iters = torch.empty(Ng, dtype=torch.int32, device=dev)
        status = torch.empty(Ng, dtype=torch.int32, device=dev)
        nu0, cov0, dec0 = torch.empty((Ng, 1), dtype=torch.float64, device=dev), torch.empty((Ng, 1), dtype=torch.float64, device=dev), \
            torch.empty(Ng, dtype=torch.float64, device=dev)
        it0, st0 = torch.empty(Ng, dtype=torch.int32, device=dev), torch.empty(Ng, dtype=torch.int32, device=dev)
        const = torch.empty(Ng, dtype=torch.float64, device=dev)
        step = int(chunk_genes) if chunk_genes is not None else default_chunk_genes(Nc)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0 in range(0, Ng, step):
            g1 = min(Ng, g0 + step)
            n = g1 - g0
            blk = _gene_block(counts, g0, g1, Nc, dev)
            lo, hi = float(blk.min()), float(blk.max())
            if not (lo >= 0.0 and np.isfinite(hi)):
                raise ValueError("counts must be finite and >= 0")
            if storage == "u16" and hi > 65535:
                raise ValueError("storage='u16' needs every count <= 65535")
            const[g0:g1] = _constants(blk, r64[g0:g1] if r64 is not None else None)
            if storage != "f32" and hi <= 65535:
                blk = blk.to(torch.int32)
                blk[blk >= 32768] -= 65536
                blk = blk.to(torch.int16)                                            # the bits of the uint16 value
                kind = _lib.VC_COUNTS_U16
            else:
                kind = _lib.VC_COUNTS_F32
            r_c = r_d[g0:g1] if r_d is not None else None
            # the fit, then the constant alone (K = 1: the null model of the likelihood-ratio statistic, under the prior's nu0 column)
            pm0 = pm_d[g0:g1, :1].contiguous() if pm_d is not None else None
            pp0 = pp_d[g0:g1, :1].contiguous() if pp_d is not None else None
            for (k_, pm_c, pp_c, outs) in (
                    (K, pm_d[g0:g1] if pm_d is not None else None, pp_d[g0:g1] if pp_d is not None else None,
                     (nu[g0:g1], cov[g0:g1], out["ll"][g0:g1], out["dec"][g0:g1], iters[g0:g1], status[g0:g1])),
                    (1, pm0, pp0, (nu0[g0:g1], cov0[g0:g1], out["ll0"][g0:g1], dec0[g0:g1], it0[g0:g1], st0[g0:g1]))):
                rc = lib.vc_gene_glm(ptr(blk), kind, n, Nc, Nc, ptr(B_d), k_, ptr(logm_d), _lib.NOISE[noisemodel], ptr(r_c), ptr(pm_c),
                                     ptr(pp_c), float(tol), int(max_iter), *[ptr(o) for o in outs], stream)
                if rc != _lib.VC_OK:
                    raise HipEngineError(f"vc_gene_glm failed ({rc}): {lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # the block and the slices outlive their launches
            del blk
        tri = torch.tril_indices(K, K)
        full = torch.zeros((Ng, K, K), dtype=torch.float64, device=dev)
        full[:, tri[0], tri[1]] = cov                                              # packed row by row: the order of tril_indices
        full[:, tri[1], tri[0]] = cov
        stds = torch.sqrt(torch.diagonal(full, dim1=1, dim2=2))
        return GeneHarmonicFit(means=nu.T.cpu().numpy().copy(), stds=stds.T.cpu().numpy().copy(), cov=full.cpu().numpy(),
                               loglik=(out["ll"] + const).cpu().numpy(), loglik_null=(out["ll0"] + const).cpu().numpy(),
                               decrement=out["dec"].cpu().numpy(), iterations=iters.cpu().numpy(), status=status.cpu().numpy())
