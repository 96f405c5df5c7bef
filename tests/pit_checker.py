"""float64 yardstick of the predictive PIT (velocycle_amd.predictive.predictive_pit, vc_predictive_pit): a dense torch restatement,
for small problems, of

    F_lo = (1/D) sum_d P(K <= k - 1 | theta_d),   F_hi = (1/D) sum_d P(K <= k | theta_d),   u = F_lo + v (F_hi - F_lo)

K ~ Poisson(e^eta) or the negative binomial with r = 1 / shape_inv and mean e^eta, eta = eta_S | eta_U of tests/pointwise_checker.py's
module text (restated here from the inputs), v the uniform of word 0 of the Philox block (seed, g << 32 | global cell, draw 0, matrix
m, stage 2, attempt 0) of tests/ppc_checker.py.  The CDF is the explicit sum of the pmf over j <= k, the pmf from its lgamma form: no
recurrence, no tail trick, nothing the device does.  `dtype` float32 evaluates the same statements in float32: "the reference's own
error", which the bar of the GPU tests is 4 x of.

ACCURACY UNIT per element, from the inputs alone:  s = eps32 (1 + A_gc) F_hi + eps32,  A the forward rounding scale of
pointwise_checker.log_probs (the magnitude sum of the terms of the log-probability of the observed count, max over draws): a CDF
anchored at a float32 log-probability inherits its relative error eps32 A, and a value in [0, 1] is not held below eps32 absolute.
The same unit serves F_lo, F_hi and u.
"""
import numpy as np
import torch

from tests import pointwise_checker as PC
from tests import ppc_checker as K

EPS32 = PC.EPS32
SAFETY = PC.SAFETY
SANITY = PC.SANITY
GOF_Z = 6.0                       # the project's goodness-of-fit bar (tests/test_ppc_cpu.py holds the count sampler to it)
QUANT = ("F_lo", "F_hi", "u")
STAGE = 2                         # Philox stage of v (0, 1: the count sampler's gamma and Poisson variates)


def etas(p):
    """{matrix: eta (D, Ng, Nc)} of a pointwise_checker.problem_of problem, in its dtype."""
    dr = p["draws"]
    xy, nu = dr["ϕxy"], dr["ν"]
    phi = torch.atan2(xy[..., 1], xy[..., 0])
    eta = torch.einsum("dgh,dch->dgc", nu, PC.basis(phi, p["H"], 0))
    if "Δν" in dr and p["Db"] is not None:
        eta = eta + torch.einsum("bc,dbg->dgc", p["Db"], dr["Δν"])
    eta = eta + p["cf"]
    out = {"S": eta}
    if p["kind"] == "velocity":
        omega = torch.einsum("dxh,dch,xc->dc", dr["νω"], PC.basis(phi, p["Hw"], 0), p["D"])
        d = torch.einsum("dgh,dch->dgc", nu, PC.basis(phi, p["H"], 1))
        zz = torch.relu(d * omega[:, None, :] + torch.exp(dr["logγg"])[:, :, None]) + 1e-5
        out["U"] = -dr["logβg"][:, :, None] + torch.log(zz) + eta
    return out


def log_pmf(j, eta, r):
    """log P(K = j) at log-mean eta; r None: Poisson, else the negative binomial's r (broadcast)."""
    if r is None:
        return j * eta - torch.exp(eta) - torch.lgamma(j + 1)
    return (torch.lgamma(r + j) - torch.lgamma(r) - torch.lgamma(j + 1) + r * torch.log(r) + j * eta - (r + j) * torch.log(r + torch.exp(eta)))


def cdf_pair(k, eta, r, budget=1 << 23):
    """(mean_d P(K <= k - 1), mean_d P(K <= k)) for counts k (Ng, Nc), eta (D, Ng, Nc), r None or (D, Ng): gene by gene the pmf on
    0 .. max k of the gene, cumulated (cells in chunks of at most `budget` pmf values)."""
    D, Ng, Nc = eta.shape
    lo, hi = torch.zeros_like(eta[0]), torch.zeros_like(eta[0])
    for g in range(Ng):
        kmax = int(k[g].max())
        j = torch.arange(kmax + 1, dtype=eta.dtype)
        rg = None if r is None else r[:, g, None, None]
        step = max(1, budget // (D * (kmax + 1)))
        for c0 in range(0, Nc, step):
            kg = k[g, c0:c0 + step].long()
            n = kg.numel()
            cum = torch.exp(log_pmf(j, eta[:, g, c0:c0 + step, None], rg)).cumsum(-1)       # (D, n, kmax + 1)
            at = lambda q: cum.gather(-1, q.clamp(min=0)[None, :, None].expand(D, n, 1))[..., 0]
            hi[g, c0:c0 + step] = at(kg).mean(0)
            lo[g, c0:c0 + step] = torch.where(kg > 0, at(kg - 1).mean(0), torch.zeros_like(hi[g, c0:c0 + step]))
    return lo, hi


def uniforms(Ng, Nc, seed, mat, cell_offset=0, dt=np.float64):
    """v (Ng, Nc) of count matrix `mat`."""
    idx = (np.arange(Ng, dtype=np.uint64)[:, None] << np.uint64(32)) | (np.uint64(cell_offset) + np.arange(Nc, dtype=np.uint64)[None, :])
    return K.uniform(K.block(seed, idx, 0, mat, STAGE, 0)[0], dt)


def evaluate(z, seed, dtype=torch.float64, cell_offset=0):
    """{matrix: {"F_lo", "F_hi", "u", "v": (Ng, Nc) in `dtype`; "s": the accuracy unit (float64 problems only)}}."""
    p = PC.problem_of(z, dtype)
    nb = p["noise"] == "NegativeBinomial"
    r = (1.0 / p["draws"]["shape_inv"]) if nb else None
    lp = PC.log_probs(p)
    out = {}
    for i, (m, eta) in enumerate(etas(p).items()):
        k = p[m]
        lo, hi = cdf_pair(k, eta, r)
        v = torch.as_tensor(uniforms(k.shape[0], k.shape[1], seed, i, cell_offset, np.float32 if dtype == torch.float32 else np.float64))
        u = lo + v * (hi - lo)
        A = lp[m][1].max(0).values
        out[m] = {"F_lo": lo, "F_hi": hi, "u": u, "v": v, "s": EPS32 * (1.0 + A.double()) * hi.double() + EPS32}
    return out


def ratios(got, e64):
    """Worst |got - float64| / s per quantity over every element of every matrix.  got: {matrix: {quantity: (Ng, Nc)}}."""
    worst = {q: 0.0 for q in QUANT}
    for m, ref in e64.items():
        for q in QUANT:
            a = torch.as_tensor(np.asarray(got[m][q])).double()
            if a.shape != ref[q].shape or not bool(torch.isfinite(a).all()):
                return {k: float("inf") for k in QUANT}
            worst[q] = max(worst[q], float(((a - ref[q]).abs() / ref["s"]).max()))
    return worst


def bins_of(u, B, dt=np.float64):
    """min(B - 1, floor(u B)) with the product formed in `dt`."""
    u = np.asarray(u, dtype=dt)
    return np.minimum(B - 1, np.floor(u * dt(B)).astype(np.int64))


def histograms(u, B, dt=np.float64):
    """(gene_hist (Ng, B), cell_hist (Nc, B)) int64 of u (Ng, Nc)."""
    b = bins_of(u, B, dt)
    Ng, Nc = b.shape
    gene = np.bincount((np.arange(Ng)[:, None] * B + b).ravel(), minlength=Ng * B).reshape(Ng, B)
    cell = np.bincount((np.arange(Nc)[None, :] * B + b).ravel(), minlength=Nc * B).reshape(Nc, B)
    return gene.astype(np.int64), cell.astype(np.int64)


def near_edge(u, s, B):
    """Elements whose float64 u lies within its own bar `s` of a bin edge j / B, 0 < j < B: (Ng, Nc) bool."""
    u, s = np.asarray(u, dtype=np.float64), np.asarray(s, dtype=np.float64)
    x = u * B
    d = np.abs(x - np.round(x)) / B
    inner = (np.round(x) > 0) & (np.round(x) < B)
    return (d <= s) & inner


def uniformity(hist):
    """(chi2, z, edge share) of integer histograms (..., B) against uniform, float64."""
    h = np.asarray(hist, dtype=np.float64)
    B = h.shape[-1]
    n = h.sum(-1)
    e = n[..., None] / B
    chi2 = ((h - e) ** 2 / e).sum(-1)
    return chi2, (chi2 - (B - 1)) / np.sqrt(2.0 * (B - 1)), (h[..., 0] + h[..., -1]) / n
