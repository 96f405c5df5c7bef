"""Float64 checker of the maximum-likelihood phase assignment (Phases.from_cycle_mle), written from the formulas, constants included:

    mu = exp(T[j,g]) * n_c^a,   T[j,g] = (zeta(phi_j) . means)[g],   phi_j = 2 pi j / bins
    Poisson            log p = k (T + a log n_c) - mu - lgamma(k + 1)
    NegativeBinomial   log p = lgamma(k + r) - lgamma(r) - lgamma(k + 1) + r log r + k (T + a log n_c) - (k + r) log(r + mu),   r = 1 / dispersion

and of how a result is judged: regret against eps32 * A_c with A_c = sum_g |log p(k_gc | best bin)|, exact bin where the float64
top-two margin is at least 8 eps32 A_c."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 8.0            # cells whose float64 top-two margin is below MARGIN * eps32 * A_c are excused from bin equality (only)
SAFETY = 4.0            # the bar over the float32 reference's own error (tests/helpers.py gives a different summation order the same)


def grid_phases(bins):
    """The reference's grid (phases.py:495), float32."""
    return (2 * np.pi * torch.arange(0, 1, 1. / bins, dtype=torch.float32))[:bins]


def fourier_basis64(phis, H):
    """[1, sin phi, cos phi, sin 2 phi, ...] in float64 (row order of utils.torch_fourier_basis)."""
    phis = phis.double()
    cols = [torch.ones_like(phis)]
    for k in range(1, H + 1):
        cols += [torch.sin(k * phis), torch.cos(k * phis)]
    return torch.stack(cols, -1)


def table64(means, bins):
    means = torch.as_tensor(np.asarray(means, dtype=np.float64))
    return fourier_basis64(grid_phases(bins), (means.shape[0] - 1) // 2) @ means          # [bins, Ng]


def logp64(counts, T, n_scounts, a, noisemodel, dispersion, chunk=64):
    """counts [Nc, Ng] (truncated to integers), T [bins, Ng] float64.  Returns (logP [bins, Nc], absP [bins, Nc]) in float64:
    the sum over genes of log p and of |log p|."""
    k_all = torch.as_tensor(np.trunc(np.asarray(counts, dtype=np.float64)))
    T = torch.as_tensor(T).double()
    logm = float(a) * torch.log(torch.as_tensor(np.asarray(n_scounts, dtype=np.float64)))
    Nc, Ng = k_all.shape
    logP = torch.empty((T.shape[0], Nc), dtype=torch.float64)
    absP = torch.empty_like(logP)
    if noisemodel == "NegativeBinomial":
        r = (1.0 / torch.as_tensor(np.asarray(dispersion, dtype=np.float64)).reshape(-1)).expand(Ng)[None, :, None]
    elif noisemodel != "Poisson":
        raise NotImplementedError("Not implemented yet, sorry")
    for c0 in range(0, Nc, chunk):
        k = k_all[c0:c0 + chunk].T[None]                                     # [1, Ng, n]
        eta = T[:, :, None] + logm[None, None, c0:c0 + chunk]                # [bins, Ng, n]
        mu = torch.exp(eta)
        if noisemodel == "Poisson":
            lp = k * eta - mu - torch.lgamma(k + 1)
        else:
            lp = torch.lgamma(k + r) - torch.lgamma(r) - torch.lgamma(k + 1) + r * torch.log(r) + k * eta - (k + r) * torch.log(r + mu)
        logP[:, c0:c0 + chunk] = lp.sum(1)
        absP[:, c0:c0 + chunk] = lp.abs().sum(1)
    return logP, absP


def judge(logP, absP, chosen):
    """chosen: int [Nc].  Returns a dict of per-cell float64 arrays: best (float64 arg-max, first of equals), A, regret_ratio
    (= regret / (eps32 A)), margin_ratio (= float64 top-two margin / (eps32 A)), excused (margin_ratio < MARGIN)."""
    chosen = torch.as_tensor(np.asarray(chosen)).long()
    best = torch.argmax(logP, 0)
    cols = torch.arange(logP.shape[1])
    top = logP[best, cols]
    A = absP[best, cols]
    regret = top - logP[chosen, cols]
    if logP.shape[0] > 1:
        second = torch.topk(logP, 2, dim=0).values[1]
        margin = top - second
    else:
        margin = torch.full_like(top, float("inf"))
    scale = EPS32 * A
    return dict(best=best.numpy(), A=A.numpy(), regret_ratio=(regret / scale).numpy(), margin_ratio=(margin / scale).numpy(),
                excused=(margin < MARGIN * scale).numpy())


def profile64(logP):
    return logP - logP.max(0, keepdim=True).values
