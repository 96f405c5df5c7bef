"""Per-gene harmonic regression given the cells' phases (the worker behind `Cycle.from_phases_mle`) on the HIP kernel `vc_gene_glm`.

The model is the one of `Phases.from_cycle_mle` (reference velocycle/phases.py:487-507), solved for the other factor:

    mu_gc = exp(nu_g . zeta(phi_c)) * n_c^a,   zeta = [1, sin phi, cos phi, sin 2 phi, ...]   (utils.torch_fourier_basis)
    Poisson            log p = k eta - mu - lgamma(k + 1)
    NegativeBinomial   log p = lgamma(k + r) - lgamma(r) - lgamma(k + 1) + r log r + k eta - (k + r) log(r + mu),   r = 1 / dispersion

For every gene the kernel maximises the log-likelihood over nu (optionally minus a Gaussian penalty per coefficient) by a damped Newton
iteration and returns nu, the inverse observed Hessian, the nu-dependent log-likelihood and how the iteration ended.  A second pass
with the constant alone gives the null model of the likelihood-ratio statistic for periodicity.

`dispersion="mle"` estimates the negative binomial's dispersion per gene as well, by alternation of `vc_gene_glm` (nu at the current r)
and `vc_gene_dispersion` (r = 1 / dispersion at that nu, a one-parameter bracketed Newton iteration inside the kernel); `gene_dispersion`
is the second half on its own, at coefficients given by the caller (an SVI-fitted `Cycle`'s means, say).

Genes are independent: they are walked in chunks, each chunk a dense [genes][cells] device block (a sparse layer is scattered into it
on the device), and the result does not depend on the chunk size bit for bit.  Cells cannot be cut.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import InitVar, dataclass

import numpy as np
import torch

from . import _lib
from .phase_mle import CHUNK_BYTES, NOISEMODELS, _is_sparse, u16_bits

MAX_HARMONICS = 3                    # csrc/vc_gene_glm.hip
STATUS = {_lib.VC_GLM_CONVERGED: "CONVERGED", _lib.VC_GLM_ROUNDING: "ROUNDING", _lib.VC_GLM_UNBOUNDED: "UNBOUNDED",
          _lib.VC_GLM_SINGULAR: "SINGULAR", _lib.VC_GLM_MAX_ITER: "MAX_ITER"}
DISPERSION_STATUS = {_lib.VC_DISP_CONVERGED: "CONVERGED", _lib.VC_DISP_ROUNDING: "ROUNDING", _lib.VC_DISP_AT_UPPER: "AT_UPPER",
                     _lib.VC_DISP_AT_LOWER: "AT_LOWER", _lib.VC_DISP_MAX_ITER: "MAX_ITER", _lib.VC_DISP_EVALUATED: "EVALUATED",
                     _lib.VC_DISP_NO_DATA: "NO_DATA"}
MLE_FIELDS = ("dispersion", "log_r_std", "dispersion_status", "rounds", "loglik_poisson", "overdispersion_p")
DISPERSION_MAX_ITER = 50             # steps of vc_gene_dispersion's bracketed Newton iteration per call
MLE_OPTIONS = {"dispersion_start": 0.3, "dispersion_prior": None, "rho_tol": 1e-6, "max_rounds": 10}


@dataclass
class GeneHarmonicFit:
    """Host float64 arrays.  means, stds: [2H+1, Ng] (rows [1, sin, cos, sin 2, ...], the layout of `Cycle.means`); cov: [Ng, 2H+1, 2H+1]
    (the inverse observed Hessian; stds = sqrt of its diagonal); loglik, loglik_null: [Ng] full log-likelihoods at the fit and at the
    fit of the constant alone; decrement: the last Newton decrement; iterations, status: int32 [Ng] (`STATUS` names the codes).
    After `dispersion="mle"` also, [Ng] each: dispersion = 1 / r of the float32 r the fit was made at; log_r_std: the standard error of
    ln r (NaN at a bound); dispersion_status (`DISPERSION_STATUS`); rounds: alternation rounds until the gene settled; loglik_poisson:
    the full log-likelihood of the Poisson fit of the same design; overdispersion_p: the p-value of `overdispersion_lr` under the
    boundary mixture (half a point mass at 0, half chi-square with one degree of freedom), 1 at AT_UPPER.  Otherwise None.  These six
    (`MLE_FIELDS`) are trailing arguments of the constructor and attributes of the object, but not among `dataclasses.fields()`: code
    that walks the fields of a fit meets arrays only, whatever the dispersion was."""
    means: np.ndarray
    stds: np.ndarray
    cov: np.ndarray
    loglik: np.ndarray
    loglik_null: np.ndarray
    decrement: np.ndarray
    iterations: np.ndarray
    status: np.ndarray
    dispersion: InitVar[np.ndarray] = None
    log_r_std: InitVar[np.ndarray] = None
    dispersion_status: InitVar[np.ndarray] = None
    rounds: InitVar[np.ndarray] = None
    loglik_poisson: InitVar[np.ndarray] = None
    overdispersion_p: InitVar[np.ndarray] = None
    bootstrap = None                 # `Cycle.from_phases_mle(bootstrap=n)` hangs its GeneHarmonicBootstrap here: an attribute, not a field

    def __post_init__(self, dispersion, log_r_std, dispersion_status, rounds, loglik_poisson, overdispersion_p):
        self.dispersion, self.log_r_std, self.dispersion_status = dispersion, log_r_std, dispersion_status
        self.rounds, self.loglik_poisson, self.overdispersion_p = rounds, loglik_poisson, overdispersion_p

    @property
    def overdispersion_lr(self):
        return None if self.loglik_poisson is None else 2.0 * (self.loglik - self.loglik_poisson)

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


@dataclass
class GeneDispersionFit:
    """Host float64 arrays [Ng] (iterations, status: int32; `DISPERSION_STATUS` names the codes).  dispersion = 1 / r of the float32 r the
    kernel hands over; log_r = ln r (float64); log_r_std = info^-1/2, the standard error of ln r (NaN at a bound); loglik: the full
    log-likelihood at log_r; score: d/d ln r of the (penalised) objective there."""
    dispersion: np.ndarray
    log_r: np.ndarray
    log_r_std: np.ndarray
    loglik: np.ndarray
    score: np.ndarray
    iterations: np.ndarray
    status: np.ndarray


def overdispersion_p_value(lr, status=None):
    """0.5 erfc(sqrt(lr / 2)): the survival function of the boundary mixture 0.5 delta_0 + 0.5 chi2_1 at lr > 0 (the Poisson model is the
    r -> infinity edge of the negative binomial); 1 where the dispersion fit ended AT_UPPER; NaN where lr is."""
    lr = np.asarray(lr, dtype=np.float64)
    p = np.array([0.5 * math.erfc(math.sqrt(max(v, 0.0) / 2.0)) if np.isfinite(v) else np.nan for v in lr.reshape(-1)]).reshape(lr.shape)
    if status is not None:
        p = np.where(np.asarray(status) == _lib.VC_DISP_AT_UPPER, 1.0, p)
    return p


def _dispersion_prior(prior, Ng):
    """(alpha, beta) of shape_inv ~ Gamma(alpha, beta), scalars or one value per gene -> two float64 [Ng] tensors (or None, None)."""
    if prior is None:
        return None, None
    if len(prior) != 2:
        raise ValueError("the dispersion prior is (alpha, beta) of shape_inv ~ Gamma(alpha, beta)")
    out = []
    for v in prior:
        t = torch.as_tensor(np.asarray(v, dtype=np.float64)).reshape(-1)
        if t.numel() not in (1, Ng):
            raise ValueError(f"the dispersion prior's alpha and beta must be scalars or one value per gene ({Ng}), got {t.numel()}")
        out.append(t.expand(Ng).contiguous())
    return out[0], out[1]


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


def _check_cells(counts, directions, n_scounts, tol, max_iter):
    """The refusals every per-gene worker makes of the counts' shape, the directions, n_scounts, tol and max_iter.  Returns
    (Nc, Ng, directions float64 [2, Nc], n_scounts float64 [Nc])."""
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
    return Nc, Ng, xy, n


def _dispersion_to_r(noisemodel, dispersion, Ng):
    """r = 1 / dispersion, float64 [Ng], of the negative binomial (dispersion: a scalar or one value per gene, > 0); None for Poisson."""
    if noisemodel != "NegativeBinomial":
        return None
    d = torch.as_tensor(np.asarray(dispersion, dtype=np.float64)).reshape(-1)
    if d.numel() not in (1, Ng):
        raise ValueError(f"dispersion must be a scalar or one value per gene ({Ng}), got {d.numel()}")
    if not bool((torch.isfinite(d) & (d > 0)).all()):
        raise ValueError("dispersion must be > 0")
    return (1.0 / d).expand(Ng).contiguous()


MAX_WEIGHT_ROWS = 65535              # csrc/vc_gene_glm_weighted.hip: rows of weights per call


def check_weights(weights, Nc, rows=None):
    """Case weights as the contiguous float32 host table [R, Nc] `vc_gene_glm_weighted` reads: finite and >= 0, R in 1..65535
    (rows=1: a vector [Nc] for `gene_harmonics`)."""
    w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float64)
    if rows == 1:
        if w.shape != (Nc,):
            raise ValueError(f"cell_weights must be one weight per cell ({Nc},), got {w.shape}")
        w = w[None, :]
    if w.ndim != 2 or w.shape[1] != Nc or w.shape[0] < 1:
        raise ValueError(f"weights must be [rows, cells] = (R, {Nc}), got {w.shape}")
    if w.shape[0] > MAX_WEIGHT_ROWS:
        raise ValueError(f"at most {MAX_WEIGHT_ROWS} rows of weights, got {w.shape[0]}")
    w32 = np.ascontiguousarray(w, dtype=np.float32)
    if not (np.isfinite(w32).all() and (w >= 0).all()):
        raise ValueError("weights must be finite and >= 0")
    return w32


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
    Nc, Ng, xy, n = _check_cells(counts, directions, n_scounts, tol, max_iter)
    r = _dispersion_to_r(noisemodel, dispersion, Ng)
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


def _constants(blk, r64, w64=None):
    """The part of every gene's log-likelihood that does not depend on nu and that the kernel leaves out, float64 [n]:
    -lgamma(k + 1), and for the negative binomial lgamma(k + r) - lgamma(r) (its r log r is inside the kernel's objective).
    w64: float64 [Nc] case weights every cell's term is multiplied by (ones change no bit)."""
    out = torch.empty(blk.shape[0], dtype=torch.float64, device=blk.device)
    rows = max(1, (1 << 24) // blk.shape[1])
    for i in range(0, blk.shape[0], rows):
        k = blk[i:i + rows].double()
        t = -torch.lgamma(k + 1.0)
        if r64 is not None:
            rr = r64[i:i + rows, None]
            t += torch.lgamma(k + rr) - torch.lgamma(rr)
        if w64 is not None:
            t = t * w64[None, :]
        out[i:i + rows] = _row_sums(t)
    return out


def _stage(counts, g0, g1, Nc, dev, storage):
    """Genes [g0, g1) on the device: (the float32 block, the block the kernels read, its count kind)."""
    blk = _gene_block(counts, g0, g1, Nc, dev)
    lo, hi = float(blk.min()), float(blk.max())
    if not (lo >= 0.0 and np.isfinite(hi)):
        raise ValueError("counts must be finite and >= 0")
    if storage == "u16" and hi > 65535:
        raise ValueError("storage='u16' needs every count <= 65535")
    if storage != "f32" and hi <= 65535:
        return blk, u16_bits(blk), _lib.VC_COUNTS_U16
    return blk, blk, _lib.VC_COUNTS_F32


def _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
    """The genes in chunks of `chunk_genes` (None: `default_chunk_genes`), each staged on the device as it is asked for: yields
    (g0, g1, the float32 block, the block the kernels read, its count kind).  Nothing here keeps a block: whoever iterates drops his
    (`del`) once the launches that read it are through, before he asks for the next."""
    if _is_sparse(counts):
        counts = counts.tocsc()
    step = int(chunk_genes) if chunk_genes is not None else default_chunk_genes(Nc)
    for g0 in range(0, Ng, step):
        g1 = min(Ng, g0 + step)
        yield (g0, g1, *_stage(counts, g0, g1, Nc, dev, storage))


def _unpack_tri(packed, K):
    """[n, K (K + 1) / 2] lower triangles packed row by row (the order of tril_indices) -> the symmetric matrices [n, K, K]."""
    tri = torch.tril_indices(K, K)
    full = torch.zeros((packed.shape[0], K, K), dtype=packed.dtype, device=packed.device)
    full[:, tri[0], tri[1]] = packed
    full[:, tri[1], tri[0]] = packed
    return full


def _check_run_options(storage, chunk_genes):
    if storage not in ("auto", "f32", "u16"):
        raise ValueError(f"unknown storage {storage!r}")
    if chunk_genes is not None and int(chunk_genes) < 1:
        raise ValueError("chunk_genes must be >= 1")


def _open_device(device):
    lib = _lib.load()
    from .engine import HipEngineError
    if not torch.cuda.is_available():
        raise HipEngineError("velocycle_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return lib, torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}"), HipEngineError


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _alternate(glm, disp, n, r, rho_tol, max_rounds, dev):
    """Alternation of one chunk: `glm(r)` fits nu [n, K] at the float32 r, `disp(nu, r)` returns (rho, r', info, status) at that nu.
    A gene is settled when its float32 r repeats bit for bit, when |delta rho| <= rho_tol, or when it sits at the same bound twice; a
    settled gene keeps its r and what the dispersion kernel said of it, whatever the other genes of the chunk still need (so that a
    gene's result does not depend on its chunk).  One read-back per round.  Returns (r, rho, info, status, rounds)."""
    active = torch.ones(n, dtype=torch.bool, device=dev)
    rho = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rounds = torch.zeros(n, dtype=torch.int32, device=dev)
    for rnd in range(1, int(max_rounds) + 1):
        rho_n, r_n, info_n, st_n = disp(glm(r), r)
        bound = (st_n == _lib.VC_DISP_AT_UPPER) | (st_n == _lib.VC_DISP_AT_LOWER)
        settled = (r_n.view(torch.int32) == r.view(torch.int32)) | ((rho_n - rho).abs() <= rho_tol) | (bound & (st_n == status))
        r = torch.where(active, r_n, r)
        rho, info, status = torch.where(active, rho_n, rho), torch.where(active, info_n, info), torch.where(active, st_n, status)
        rounds = torch.where(active, torch.full_like(rounds, rnd), rounds)
        active = active & ~settled
        if not bool(active.any()):
            break
    return r.contiguous(), rho, info, status, rounds


def gene_harmonics(counts, directions, n_scounts, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, *, prior_means=None,
                   prior_stds=None, tol=1e-10, max_iter=25, device=None, chunk_genes=None, storage="auto", **mle_options):
    """counts: [Nc, Ng] cell-major like an AnnData layer (numpy, scipy sparse or torch); directions: [2, Nc] phase directions (rows x, y
    like `Phases.phi_xy`, any length > 0); n_scounts: [Nc] > 0; dispersion: scalar or [Ng]; prior_means / prior_stds: [2H+1, Ng] like
    `Cycle.means` / `Cycle.stds` (a coefficient with a non-finite mean or std has no prior).  storage: "auto" (uint16 per chunk when every
    count is an integer <= 65535) | "f32" | "u16".  Returns a `GeneHarmonicFit`.

    dispersion="mle" (NegativeBinomial only) estimates the dispersion of every gene with its harmonics, by alternation from
    `dispersion_start` (0.3; scalar or [Ng]): per round `vc_gene_glm` at the current float32 r, then `vc_gene_dispersion` at its nu, until
    every gene of the chunk is settled (`_alternate`) or `max_rounds` (10) rounds are spent, then `vc_gene_glm` once more at the final r.
    `dispersion_prior=(alpha, beta)` puts shape_inv ~ Gamma(alpha, beta) on the dispersion; `rho_tol` (1e-6) is the settling tolerance of
    ln r.  The null model has its own alternation, so `lr_stat` compares two maximised likelihoods.  These four are accepted by name only
    and do nothing when `dispersion` is a number or an array.

    cell_weights (accepted by name only, default None): [Nc] finite case weights >= 0 (float32 on the device): every cell's term of the log-likelihood, of its
    gradient and of its Hessian is multiplied by its weight, in the fit and in the null model alike, on the kernel
    `vc_gene_glm_weighted` (one row of weights); `loglik` and `loglik_null` carry the weighted constants, `lr_stat` and `p_value` follow
    from them.  A vector of ones returns the unweighted result bit for bit.  A gene without a count in any cell of positive weight ends
    UNBOUNDED.  `dispersion="mle"` with weights is refused: `vc_gene_dispersion` knows no weights (nor does the kinetics
    worker; the batch worker has them: `gene_batch.gene_harmonics_batched(cell_weights=)`).  `gene_bootstrap.gene_harmonics_bootstrap` solves many rows of weights per call."""
    cell_weights = mle_options.pop("cell_weights", None)                             # by name only, like the options of "mle"
    if cell_weights is not None and isinstance(dispersion, str):
        raise ValueError("cell_weights with dispersion='mle' is not supported: vc_gene_dispersion knows no weights")
    unknown = set(mle_options) - set(MLE_OPTIONS)
    if unknown:
        raise TypeError(f"gene_harmonics() got unexpected keyword arguments {sorted(unknown)}")
    opt = {**MLE_OPTIONS, **mle_options}
    mle = isinstance(dispersion, str)
    if mle:
        if dispersion != "mle":
            raise ValueError(f"dispersion must be a number, one number per gene, or 'mle', got {dispersion!r}")
        if noisemodel == "Poisson":
            raise ValueError("dispersion='mle' needs noisemodel='NegativeBinomial': the Poisson model has no dispersion")
        if not (opt["rho_tol"] >= 0):
            raise ValueError("rho_tol must be >= 0")
        if int(opt["max_rounds"]) != opt["max_rounds"] or opt["max_rounds"] < 1:
            raise ValueError("max_rounds must be an integer >= 1")
    basis, logm, r, pm, pp = check_arguments(counts, directions, n_scounts, harmonics, a, noisemodel,
                                             opt["dispersion_start"] if mle else dispersion, prior_means, prior_stds, tol, max_iter)
    _check_run_options(storage, chunk_genes)
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    w_host = check_weights(cell_weights, Nc, rows=1) if cell_weights is not None else None
    pa, pb = _dispersion_prior(opt["dispersion_prior"], Ng) if mle else (None, None)
    lib, dev, HipEngineError = _open_device(device)
    K = basis.shape[0]
    NH = K * (K + 1) // 2
    ptr = _ptr
    with torch.cuda.device(dev):
        w_d = torch.from_numpy(w_host).to(dev).contiguous() if w_host is not None else None
        w64 = w_d[0].double() if w_d is not None else None
        B_d = basis.to(torch.float32).to(dev).contiguous()
        logm_d = logm.to(torch.float32).to(dev).contiguous()
        r_d = r.to(torch.float32).to(dev).contiguous() if r is not None else None
        r64 = r_d.double() if r_d is not None else None                          # the model is the one of the float32 r the kernel reads
        pm_d = pm.to(dev).contiguous() if pm is not None else None
        pp_d = pp.to(dev).contiguous() if pp is not None else None
        pa_d = pa.to(dev).contiguous() if pa is not None else None
        pb_d = pb.to(dev).contiguous() if pb is not None else None
        nu = torch.empty((Ng, K), dtype=torch.float64, device=dev)
        cov = torch.empty((Ng, NH), dtype=torch.float64, device=dev)
        out = {n: torch.empty(Ng, dtype=torch.float64, device=dev) for n in ("ll", "dec", "ll0")}
        iters = torch.empty(Ng, dtype=torch.int32, device=dev)
        status = torch.empty(Ng, dtype=torch.int32, device=dev)
        nu0, cov0, dec0 = torch.empty((Ng, 1), dtype=torch.float64, device=dev), torch.empty((Ng, 1), dtype=torch.float64, device=dev), \
            torch.empty(Ng, dtype=torch.float64, device=dev)
        it0, st0 = torch.empty(Ng, dtype=torch.int32, device=dev), torch.empty(Ng, dtype=torch.int32, device=dev)
        const = torch.empty(Ng, dtype=torch.float64, device=dev)
        const0 = const
        if mle:
            const0 = torch.empty(Ng, dtype=torch.float64, device=dev)
            extra = {n: torch.empty(Ng, dtype=torch.float64, device=dev) for n in ("r", "rho", "info", "llp", "constp")}
            dstatus = torch.empty(Ng, dtype=torch.int32, device=dev)
            rounds = torch.empty(Ng, dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0, g1, blk, kblk, kind in _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
            n = g1 - g0

            def glm(k_, noise, r_c, pm_c, pp_c, outs):
                if w_d is not None:                                              # one row of case weights, each gene from its default start
                    rc = lib.vc_gene_glm_weighted(ptr(kblk), kind, n, Nc, Nc, ptr(B_d), k_, ptr(logm_d), _lib.NOISE[noise], ptr(r_c),
                                                  ptr(pm_c), ptr(pp_c), ptr(w_d), 1, Nc, None, float(tol), int(max_iter),
                                                  *[ptr(o) for o in outs], stream)
                    if rc != _lib.VC_OK:
                        raise HipEngineError(f"vc_gene_glm_weighted failed ({rc}): {lib.vc_last_error(None).decode()}")
                    return
                rc = lib.vc_gene_glm(ptr(kblk), kind, n, Nc, Nc, ptr(B_d), k_, ptr(logm_d), _lib.NOISE[noise], ptr(r_c), ptr(pm_c),
                                     ptr(pp_c), float(tol), int(max_iter), *[ptr(o) for o in outs], stream)
                if rc != _lib.VC_OK:
                    raise HipEngineError(f"vc_gene_glm failed ({rc}): {lib.vc_last_error(None).decode()}")

            # the fit, then the constant alone (K = 1: the null model of the likelihood-ratio statistic, under the prior's nu0 column)
            pm0 = pm_d[g0:g1, :1].contiguous() if pm_d is not None else None
            pp0 = pp_d[g0:g1, :1].contiguous() if pp_d is not None else None
            models = ((K, pm_d[g0:g1] if pm_d is not None else None, pp_d[g0:g1] if pp_d is not None else None,
                       (nu[g0:g1], cov[g0:g1], out["ll"][g0:g1], out["dec"][g0:g1], iters[g0:g1], status[g0:g1])),
                      (1, pm0, pp0, (nu0[g0:g1], cov0[g0:g1], out["ll0"][g0:g1], dec0[g0:g1], it0[g0:g1], st0[g0:g1])))
            if not mle:
                const[g0:g1] = _constants(blk, r64[g0:g1] if r64 is not None else None, w64)
                r_c = r_d[g0:g1] if r_d is not None else None
                for (k_, pm_c, pp_c, outs) in models:
                    glm(k_, noisemodel, r_c, pm_c, pp_c, outs)
            else:
                pa_c = pa_d[g0:g1] if pa_d is not None else None
                pb_c = pb_d[g0:g1] if pb_d is not None else None
                dd = {n_: torch.empty(n, dtype=torch.float64, device=dev) for n_ in ("rho", "info", "ll", "score")}
                dr = torch.empty(n, dtype=torch.float32, device=dev)
                di, ds = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
                for (k_, pm_c, pp_c, outs), cst in zip(models, (const, const0)):
                    def fit_nu(r_c):
                        glm(k_, noisemodel, r_c, pm_c, pp_c, outs)
                        return outs[0]

                    def fit_r(nu_c, r_c):
                        rc = lib.vc_gene_dispersion(ptr(kblk), kind, n, Nc, Nc, ptr(B_d), k_, ptr(logm_d), ptr(nu_c), ptr(r_c), ptr(pa_c),
                                                    ptr(pb_c), float(tol), DISPERSION_MAX_ITER, ptr(dd["rho"]), ptr(dr), ptr(dd["info"]), ptr(dd["ll"]),
                                                    ptr(dd["score"]), ptr(di), ptr(ds), stream)
                        if rc != _lib.VC_OK:
                            raise HipEngineError(f"vc_gene_dispersion failed ({rc}): {lib.vc_last_error(None).decode()}")
                        return dd["rho"].clone(), dr.clone(), dd["info"].clone(), ds.clone()

                    r_c, rho_c, info_c, st_c, rounds_c = _alternate(fit_nu, fit_r, n, r_d[g0:g1].clone(), float(opt["rho_tol"]),
                                                                    opt["max_rounds"], dev)
                    fit_nu(r_c)                                                  # means, cov and loglik are those of the reported r
                    cst[g0:g1] = _constants(blk, r_c.double())
                    if k_ == K:
                        extra["r"][g0:g1], extra["rho"][g0:g1], extra["info"][g0:g1] = r_c.double(), rho_c, info_c
                        dstatus[g0:g1], rounds[g0:g1] = st_c, rounds_c
                # the Poisson fit of the same design: the r -> infinity edge the overdispersion test compares with
                tmp = (torch.empty((n, K), dtype=torch.float64, device=dev), torch.empty((n, NH), dtype=torch.float64, device=dev),
                       extra["llp"][g0:g1], dd["score"], di, ds)
                glm(K, "Poisson", None, models[0][1], models[0][2], tmp)
                extra["constp"][g0:g1] = _constants(blk, None)
            torch.cuda.current_stream(dev).synchronize()                             # the block and the slices outlive their launches
            del blk, kblk
        full = _unpack_tri(cov, K)
        stds = torch.sqrt(torch.diagonal(full, dim1=1, dim2=2))
        fit = GeneHarmonicFit(means=nu.T.cpu().numpy().copy(), stds=stds.T.cpu().numpy().copy(), cov=full.cpu().numpy(),
                              loglik=(out["ll"] + const).cpu().numpy(), loglik_null=(out["ll0"] + const0).cpu().numpy(),
                              decrement=out["dec"].cpu().numpy(), iterations=iters.cpu().numpy(), status=status.cpu().numpy())
        if mle:
            fit.dispersion = (1.0 / extra["r"]).cpu().numpy()
            fit.log_r_std = _info_to_std(extra["info"].cpu().numpy())
            fit.dispersion_status = dstatus.cpu().numpy()
            fit.rounds = rounds.cpu().numpy()
            fit.loglik_poisson = (extra["llp"] + extra["constp"]).cpu().numpy()
            fit.overdispersion_p = overdispersion_p_value(fit.overdispersion_lr, fit.dispersion_status)
        return fit


def _info_to_std(info):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(info > 0, 1.0 / np.sqrt(np.where(info > 0, info, 1.0)), np.nan)


def gene_dispersion(counts, directions, n_scounts, means, a=1, *, start=None, prior=None, tol=1e-10, max_iter=DISPERSION_MAX_ITER,
                    evaluate_only=False,
                    device=None, chunk_genes=None, storage="auto"):
    """The negative-binomial dispersion of every gene at given coefficients `means` ([2H+1, Ng] like `Cycle.means`, e.g. those of an
    SVI-fitted cycle), on the HIP kernel `vc_gene_dispersion`: the maximum over ln r (r = 1 / dispersion, within [1e-3, 1e6]) of the
    log-likelihood, or with `prior=(alpha, beta)` the mode under shape_inv ~ Gamma(alpha, beta).  counts, directions, n_scounts, a,
    device, chunk_genes, storage: as for `gene_harmonics` (same staging, chunking and truncation).  start: a dispersion (scalar or [Ng])
    the iteration starts from (None: the moment estimate); evaluate_only=True makes one pass at `start` and returns the log-likelihood,
    the score and the curvature there.  Returns a `GeneDispersionFit`."""
    nu = np.asarray(means, dtype=np.float64)
    if nu.ndim != 2 or nu.shape[0] not in (1, 3, 5, 7):
        raise ValueError(f"means must be [2 harmonics + 1, genes] with 0..{MAX_HARMONICS} harmonics, got {nu.shape}")
    if len(counts.shape) == 2 and nu.shape[1] != counts.shape[1]:
        raise ValueError(f"means has {nu.shape[1]} genes, counts {counts.shape[1]}")
    if evaluate_only and start is None:
        raise ValueError("evaluate_only needs start: the dispersion to evaluate at")
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError("max_iter must be an integer >= 1")
    basis, logm, r, _, _ = check_arguments(counts, directions, n_scounts, (nu.shape[0] - 1) // 2, a, "NegativeBinomial",
                                           0.3 if start is None else start, None, None, tol, max_iter)
    _check_run_options(storage, chunk_genes)
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    pa, pb = _dispersion_prior(prior, Ng)
    lib, dev, HipEngineError = _open_device(device)
    K = basis.shape[0]
    ptr = _ptr
    with torch.cuda.device(dev):
        B_d = basis.to(torch.float32).to(dev).contiguous()
        logm_d = logm.to(torch.float32).to(dev).contiguous()
        nu_d = torch.as_tensor(np.ascontiguousarray(nu.T)).to(dev)
        r_d = r.to(torch.float32).to(dev).contiguous() if start is not None else None
        pa_d = pa.to(dev).contiguous() if pa is not None else None
        pb_d = pb.to(dev).contiguous() if pb is not None else None
        out = {n: torch.empty(Ng, dtype=torch.float64, device=dev) for n in ("rho", "info", "ll", "score", "const")}
        r_out = torch.empty(Ng, dtype=torch.float32, device=dev)
        iters = torch.empty(Ng, dtype=torch.int32, device=dev)
        status = torch.empty(Ng, dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for g0, g1, blk, kblk, kind in _chunks(counts, Nc, Ng, dev, storage, chunk_genes):
            out["const"][g0:g1] = _constants(blk, None)
            sl = lambda t: t[g0:g1] if t is not None else None                       # noqa: E731
            rc = lib.vc_gene_dispersion(ptr(kblk), kind, g1 - g0, Nc, Nc, ptr(B_d), K, ptr(logm_d), ptr(nu_d[g0:g1]), ptr(sl(r_d)),
                                        ptr(sl(pa_d)), ptr(sl(pb_d)), float(tol), 0 if evaluate_only else int(max_iter),
                                        ptr(out["rho"][g0:g1]), ptr(r_out[g0:g1]), ptr(out["info"][g0:g1]), ptr(out["ll"][g0:g1]),
                                        ptr(out["score"][g0:g1]), ptr(iters[g0:g1]), ptr(status[g0:g1]), stream)
            if rc != _lib.VC_OK:
                raise HipEngineError(f"vc_gene_dispersion failed ({rc}): {lib.vc_last_error(None).decode()}")
            torch.cuda.current_stream(dev).synchronize()                             # the block outlives its launch
            del blk, kblk
        return GeneDispersionFit(dispersion=(1.0 / r_out.double()).cpu().numpy(), log_r=out["rho"].cpu().numpy(),
                                 log_r_std=_info_to_std(out["info"].cpu().numpy()), loglik=(out["ll"] + out["const"]).cpu().numpy(),
                                 score=out["score"].cpu().numpy(), iterations=iters.cpu().numpy(), status=status.cpu().numpy())
