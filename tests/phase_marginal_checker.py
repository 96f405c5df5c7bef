"""float64 yardstick of phase-marginal scoring (velocycle_amd.predictive.phase_marginal, vc_phase_marginal): a dense torch restatement
for small problems, built from tests/pointwise_checker.py::log_probs evaluated with every cell's direction set to the grid phase
phi_j = 2 pi j / B:

    a[d,c,j]      = lw[c,j] + sum_matrices sum_g log p(k_gc | theta_d, phi_j)
    evidence[c]   = log((1/D) sum_d sum_j exp a),   post[c,j] = sum_d exp a[d,c,j] / sum_d sum_j' exp a[d,c,j'],
    per_draw[d,c] = log sum_j exp a[d,c,j]

together with a FORWARD ROUNDING SCALE per cell, from the inputs alone: A_c = max_{d,j} sum_matrices sum_g A_gc, A_gc the pointwise
checker's term-magnitude scale with its kink amplification.  Units of an error: evidence and per_draw eps32 A_c; post
eps32 A_c post + eps32 (a relative error of eps32 A_c on the bin's mass and one float32 rounding of the stored value).
It shares no code with the device; the simulator below (`means`, `simulate`) restates the model a second time for the calibration tests."""
import math

import numpy as np
import torch

from tests import pointwise_checker as PC

EPS32 = PC.EPS32
QUANT = ("evidence", "post", "per_draw")
MAX_ELEMENTS = 1 << 22            # draws x genes x (cells x bins of one pass): the bins are walked in groups of this size


def grid(B, dtype=torch.float64):
    return 2.0 * math.pi * torch.arange(B, dtype=torch.float64).to(dtype) / B


def _tile_cells(p, nb):
    q = dict(p)
    rep = lambda t, ax: None if t is None else torch.cat([t] * nb, dim=ax)
    q["S"], q["U"], q["cf"], q["Db"], q["D"] = rep(p["S"], 1), rep(p["U"], 1), rep(p["cf"], 0), rep(p["Db"], 1), rep(p["D"], 1)
    return q


def gene_sums(p, B):
    """(sum over matrices and genes of log p, the same of the term-magnitude scale), each (D, Nc, B), in the dtype of the problem."""
    dr = p["draws"]
    D, Ng = dr["ν"].shape[0], p["S"].shape[0]
    Nc = p["S"].shape[1]
    dtype = p["S"].dtype
    phis = grid(B)
    per = max(1, MAX_ELEMENTS // max(1, D * Ng * Nc))
    tot = torch.empty((D, Nc, B), dtype=dtype)
    scale = torch.empty((D, Nc, B), dtype=dtype)
    for j0 in range(0, B, per):
        nb = min(per, B - j0)
        q = _tile_cells(p, nb)
        ph = phis[j0:j0 + nb].repeat_interleave(Nc)                             # bin-major: column jj * Nc + c
        xy = torch.stack([torch.cos(ph), torch.sin(ph)], dim=-1).to(dtype)
        q["draws"] = dict(dr, **{"ϕxy": xy.expand(D, nb * Nc, 2)})
        l_sum, a_sum = 0.0, 0.0
        for l, a in PC.log_probs(q).values():
            l_sum = l_sum + l.sum(1)
            a_sum = a_sum + a.sum(1)
        tot[:, :, j0:j0 + nb] = l_sum.reshape(D, nb, Nc).transpose(1, 2)
        scale[:, :, j0:j0 + nb] = a_sum.reshape(D, nb, Nc).transpose(1, 2)
    return tot, scale


def evaluate_problem(p, B, lw=None):
    """{"evidence": (Nc,), "post": (Nc, B), "per_draw": (D, Nc), "A": (Nc,)} of a problem (pointwise_checker.problem_of) in its dtype.
    lw: (Nc, B) log prior masses, or None: flat, -log B."""
    tot, scale = gene_sums(p, B)
    dtype = tot.dtype
    D = tot.shape[0]
    lwt = torch.full(tot.shape[1:], -math.log(B), dtype=dtype) if lw is None else torch.as_tensor(np.asarray(lw)).to(dtype)
    a = tot + lwt
    per_draw = torch.logsumexp(a, dim=2)
    bins = torch.logsumexp(a, dim=0)                                            # (Nc, B) log mass of every bin
    total = torch.logsumexp(bins, dim=1)
    return {"evidence": total - math.log(D), "post": torch.exp(bins - total[:, None]), "per_draw": per_draw, "A": scale.amax(dim=(0, 2))}


def evaluate(z, B, lw=None, dtype=torch.float64):
    return evaluate_problem(PC.problem_of(z, dtype), B, lw)


def ratios(got, e64):
    """Worst error ratio per quantity of `got` ({"evidence", "post", "per_draw"?} of array-likes) against the float64 evaluation; every
    element takes part; a non-finite value gives inf."""
    A = e64["A"].double()
    units = {"evidence": EPS32 * A, "per_draw": (EPS32 * A)[None, :].expand_as(e64["per_draw"]),
             "post": EPS32 * A[:, None] * e64["post"].double() + EPS32}
    out = {}
    for q in QUANT:
        if got.get(q) is None:
            continue
        g = torch.as_tensor(np.asarray(got[q])).double()
        assert g.shape == e64[q].shape, (q, g.shape, e64[q].shape)
        out[q] = float(((g - e64[q].double()).abs() / units[q]).max()) if bool(torch.isfinite(g).all()) else float("inf")
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# calibration: counts simulated from the model at a known grid phase, the randomized PIT of the true bin under the posterior
# ----------------------------------------------------------------------------------------------------------------------------------
def means(p, phi, d=0):
    """(mu_S, mu_U | None), each (Ng, Nc): the model's means under draw d with the cells at the phases phi (Nc,)."""
    dr = p["draws"]
    nu = dr["ν"][d]
    eta = nu @ PC.basis(phi, p["H"], 0).T
    if "Δν" in dr and p["Db"] is not None:
        eta = eta + dr["Δν"][d].T @ p["Db"]
    eta = eta + p["cf"][None, :]
    if p["kind"] != "velocity":
        return torch.exp(eta), None
    omega = ((dr["νω"][d] @ PC.basis(phi, p["Hw"], 0).T) * p["D"]).sum(0)
    dd = nu @ PC.basis(phi, p["H"], 1).T
    zz = torch.relu(dd * omega[None, :] + torch.exp(dr["logγg"][d])[:, None]) + 1e-5
    return torch.exp(eta), torch.exp(eta - dr["logβg"][d][:, None]) * zz


def simulate(z, B, seed, d=0):
    """A copy of the fixture `z` with one draw (draw d of every site) and S (and U) drawn from the model with every cell at a phase of
    the grid, and those bins: (fixture, true_bin (Nc,))."""
    gen = torch.Generator().manual_seed(int(seed))
    p = PC.problem_of(z)
    Nc = p["S"].shape[1]
    jstar = torch.randint(0, B, (Nc,), generator=gen)
    mS, mU = means(p, grid(B)[jstar], d)

    def draw(mu):
        if p["noise"] == "NegativeBinomial":
            r = (1.0 / p["draws"]["shape_inv"][d])[:, None].expand_as(mu).contiguous()
            mu = torch._standard_gamma(r, generator=gen) / r * mu
        return torch.poisson(mu, generator=gen).numpy().astype(np.float32)
    out = dict(z)
    out["in_S"] = draw(mS)
    if mU is not None:
        out["in_U"] = draw(mU)
    for k in list(out):
        if k.startswith("draw_"):
            out[k] = np.ascontiguousarray(out[k][d:d + 1] if out[k].shape[0] > 1 else out[k])
    out["n_draws"] = np.int64(1)
    return out, jstar


def pit_z(post, jstar, seed, bins=10):
    """z-score (chi2 - (bins - 1)) / sqrt(2 (bins - 1)) of the `bins`-bin histogram of u = sum_{j<j*} post_j + v post_j*."""
    post = torch.as_tensor(np.asarray(post)).double()
    v = torch.rand(post.shape[0], generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)
    cum = torch.cumsum(post, 1)
    at = post.gather(1, jstar[:, None])[:, 0]
    u = (cum.gather(1, jstar[:, None])[:, 0] - at) + v * at
    h = torch.histc(u.clamp(0.0, 1.0 - 1e-12), bins=bins, min=0.0, max=1.0)
    e = post.shape[0] / bins
    chi2 = float((((h - e) ** 2) / e).sum())
    return (chi2 - (bins - 1)) / math.sqrt(2.0 * (bins - 1))


def wrong_models(z):
    """The two controls as fixtures: the harmonic coefficients of nu doubled; its sin and cos coefficients swapped."""
    out = []
    for kind in ("doubled", "swapped"):
        q = dict(z)
        nu = z["draw_ν"].copy()
        if kind == "doubled":
            nu[..., 1:] = 2.0 * nu[..., 1:]
        else:
            nu[..., 1::2], nu[..., 2::2] = z["draw_ν"][..., 2::2], z["draw_ν"][..., 1::2]
        q["draw_ν"] = nu
        out.append((kind, q))
    return out
