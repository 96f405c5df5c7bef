"""float64 yardstick of the pointwise predictive density (velocycle_amd.predictive, vc_pointwise_density): a dense torch restatement
for small problems of

    eta_S = nu_d[g,:] . zeta(phi_dc) + sum_b Db[b,c] dnu[b,g] + count_factor[c]
    omega = sum_x sum_h nuomega_d[x,h] zeta_omega_h(phi_dc) D[x,c]
    z     = (nu_d[g,:] . zeta'(phi_dc)) omega + exp(loggamma_d[g]);  eta_U = -logbeta_d[g] + log(relu(z) + 1e-5) + eta_S
    NegativeBinomial  l = lgamma(r+k) - lgamma(r) - lgamma(k+1) + r log r + k eta - (r+k) log(r + e^eta),  r = 1 / shape_inv[g]
    Poisson           l = k eta - e^eta - lgamma(k+1)
    lppd = log mean_d exp l_d,   mean = mean_d l_d,   pwaic = sum_d (l_d - mean)^2 / (D - 1)

together with a FORWARD ROUNDING SCALE per element, computed from the inputs alone: A_gc = max_d of the sum of the magnitudes of the
terms of l_d, plus for U the first-order amplification of the kink argument, |dl / d log(relu(z) + 1e-5)| (|d omega| + gamma) /
(relu(z) + 1e-5) with d = nu . zeta'.  Scales of sums are the sums of the element scales.  The error of a result is
|result - float64| / (eps32 A); for pwaic the scale is 2 sigma eps32 A + (eps32 A)^2 per element, summed likewise.
"""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
SAFETY = 4.0                     # tests/mle_checker.SAFETY: the margin of a float32 GPU evaluation over a float32 CPU one
SANITY = 64.0                    # the band the float32 reference itself must stay in on every fixture
SITES = ("ϕxy", "ν", "Δν", "shape_inv", "logγg", "logβg", "νω")
QUANT = ("lppd", "mean", "pwaic")


def basis(phi, H, der=0):
    """[1, sin p, cos p, sin 2p, ...] (der = 0) or its derivative; (..., Nc) -> (..., Nc, 2H+1)."""
    cols = [torch.ones_like(phi) if der == 0 else torch.zeros_like(phi)]
    for k in range(1, H + 1):
        cols += [torch.sin(k * phi), torch.cos(k * phi)] if der == 0 else [k * torch.cos(k * phi), -k * torch.sin(k * phi)]
    return torch.stack(cols, dim=-1)


def _f(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def problem_of(z, dtype=torch.float64):
    """The inputs of a fixture (keys `in_*` as tests/helpers reads them, `draw_<site>` = (D or 1, *site shape)) as tensors of `dtype`."""
    p = dict(kind=str(z["in_kind"]), noise=str(z["in_noisemodel"]), H=int(z["in_H"]), Hw=int(z["in_Hw"]) if "in_Hw" in z else 0)
    vel = p["kind"] == "velocity"
    p["S"] = _f(z["in_S"], dtype)
    p["U"] = _f(z["in_U"], dtype) if vel else None
    p["cf"] = _f(z["in_count_factor"], dtype).reshape(-1)
    p["Db"] = _f(z["in_Db"], dtype) if bool(z["in_with_delta_nu"]) else None
    p["D"] = _f(z["in_D"], dtype) if vel else None
    D = max(int(np.asarray(z["draw_" + s]).shape[0]) for s in SITES if "draw_" + s in z)
    p["draws"] = {}
    for s in SITES:
        if "draw_" + s in z:
            t = _f(z["draw_" + s], dtype)
            p["draws"][s] = t.expand((D,) + tuple(t.shape[1:])) if t.shape[0] == 1 else t
    return p


def log_probs(p):
    """Per matrix: l (D, Ng, Nc) and the magnitude sum of its terms (D, Ng, Nc), in the dtype of the problem."""
    dr = p["draws"]
    xy, nu = dr["ϕxy"], dr["ν"]
    phi = torch.atan2(xy[..., 1], xy[..., 0])                                  # (D, Nc)
    zeta = basis(phi, p["H"], 0)
    eta = torch.einsum("dgh,dch->dgc", nu, zeta)
    if "Δν" in dr and p["Db"] is not None:
        eta = eta + torch.einsum("bc,dbg->dgc", p["Db"], dr["Δν"])
    eta = eta + p["cf"]
    nb = p["noise"] == "NegativeBinomial"
    r = (1.0 / dr["shape_inv"])[:, :, None] if nb else None

    def lik(k, e):
        if nb:
            t = [torch.lgamma(r + k), -torch.lgamma(r) + 0 * e, -torch.lgamma(k + 1) + 0 * e, r * torch.log(r) + 0 * e, k * e,
                 -(r + k) * torch.log(r + torch.exp(e))]
            dl = k - (r + k) * torch.exp(e) / (r + torch.exp(e))
        else:
            t = [k * e, -torch.exp(e), -torch.lgamma(k + 1) + 0 * e]
            dl = k - torch.exp(e)
        return sum(t), sum(x.abs() for x in t), dl

    out = {}
    l, a, _ = lik(p["S"], eta)
    out["S"] = (l, a)
    if p["kind"] == "velocity":
        zd = basis(phi, p["H"], 1)
        zw = basis(phi, p["Hw"], 0)
        omega = torch.einsum("dxh,dch,xc->dc", dr["νω"], zw, p["D"])
        d = torch.einsum("dgh,dch->dgc", nu, zd)
        gam = torch.exp(dr["logγg"])[:, :, None]
        zz = torch.relu(d * omega[:, None, :] + gam) + 1e-5
        eu = -dr["logβg"][:, :, None] + torch.log(zz) + eta
        l, a, dl = lik(p["U"], eu)
        a = a + dl.abs() * ((d * omega[:, None, :]).abs() + gam) / zz
        out["U"] = (l, a)
    return out


def reduce_draws(l):
    """(lppd, mean, pwaic) per element of l (D, Ng, Nc): log-sum-exp around the maximum, mean shifted by the first draw (equal draws
    give lppd == mean exactly and pwaic == 0), centred second moment."""
    D = l.shape[0]
    m = l.max(0).values
    lppd = m + torch.log(torch.exp(l - m).sum(0) / D)
    mean = l[0] + (l - l[0]).mean(0)
    pwaic = ((l - mean) ** 2).sum(0) / (D - 1)
    return lppd, mean, pwaic


def evaluate(z, dtype=torch.float64):
    """{matrix: {"lppd" | "mean" | "pwaic": (Ng, Nc), "A": (Ng, Nc)}} in `dtype` (A only meaningful in float64)."""
    p = problem_of(z, dtype)
    out = {}
    for m, (l, a) in log_probs(p).items():
        lppd, mean, pw = reduce_draws(l)
        out[m] = {"lppd": lppd, "mean": mean, "pwaic": pw, "A": a.max(0).values}
    return out


def scales(e64):
    """Per matrix and quantity the element scale (Ng, Nc) in absolute units: eps32 A, and for pwaic 2 sigma eps32 A + (eps32 A)^2."""
    out = {}
    for m, v in e64.items():
        ea = EPS32 * v["A"]
        out[m] = {"lppd": ea, "mean": ea, "pwaic": 2 * torch.sqrt(v["pwaic"]) * ea + ea ** 2}
    return out


def sums(dense):
    """{matrix: {quantity: {"gene": (Ng,), "cell": (Nc,)}}} of a {matrix: {quantity: (Ng, Nc)}}."""
    return {m: {q: {"gene": v[q].sum(1), "cell": v[q].sum(0)} for q in QUANT} for m, v in dense.items()}


def ratios(got, e64):
    """Worst error ratio per quantity of `got` against the float64 evaluation, over the dense values (where `got` has them), the
    per-gene and the per-cell sums of every matrix.  got: {matrix: {quantity: {"dense"?, "gene", "cell"}}} of array-likes."""
    sc, ref = scales(e64), sums(e64)
    ssc = sums(sc)
    worst = {q: 0.0 for q in QUANT}
    for m in e64:
        for q in QUANT:
            g = got[m][q]
            pairs = [(g["gene"], ref[m][q]["gene"], ssc[m][q]["gene"]), (g["cell"], ref[m][q]["cell"], ssc[m][q]["cell"])]
            if g.get("dense") is not None:
                pairs.append((g["dense"], e64[m][q], sc[m][q]))
            for a, b, s in pairs:
                a = torch.as_tensor(np.asarray(a)).double()
                if not bool(torch.isfinite(a).all()):
                    return {k: float("inf") for k in QUANT}
                err = (a - b).abs()
                ok = s > 0
                if bool((err[~ok] > 0).any()):
                    return {k: float("inf") for k in QUANT}
                if bool(ok.any()):
                    worst[q] = max(worst[q], float((err[ok] / s[ok]).max()))
    return worst


def as_got(dense):
    """A dense evaluation {matrix: {quantity: (Ng, Nc)}} in the form `ratios` takes (dense values and both families of sums)."""
    s = sums(dense)
    return {m: {q: {"dense": dense[m][q], "gene": s[m][q]["gene"], "cell": s[m][q]["cell"]} for q in QUANT} for m in dense}
