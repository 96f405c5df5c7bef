"""Yardstick of the posterior predictive check (velocycle_amd.predictive.predictive_check / sample_counts, csrc/vc_count_sampler.h,
csrc/vc_ppc.hip): a numpy restatement of Philox4x32-10 and of the documented count sampler, the dense eta of a
fixture's draws, and the statistics / p-values of replicated counts.

The arithmetic dtype of the sampler is a parameter: float64 is the checker, float32 "the reference's own error" -- the same operations
in the same order with one float32 rounding each, which is what the device performs (its exp2 / log2 are the hardware's).  PTRS's full
acceptance test is float64 under either dtype, from the inputs the dtype produced, as on the device.  Where a
float32 evaluation lands on the other side of an accept / floor / search decision than the float64 one, the count differs: the share
of such elements between the two restatements, times SAFETY, caps the share the device may differ from the float64 checker by.

Against the exact pmf of torch.distributions (nothing shared with the sampler): exact_moments / moment_z and the chi-square gof_z, over
GRID (rates up to 400) and LARGE_GRID (rates up to the documented 2^20).
"""
from functools import lru_cache
import math

import numpy as np
import torch

from tests import pointwise_checker as PC

SAFETY = PC.SAFETY                # a float32 GPU evaluation on hardware transcendentals over a float32 CPU one (mle_checker.SAFETY)
FLOOR = 16                        # elements: the cap's floor
MU_MAX = 1048576.0                # VC_CS_MU_MAX
SMALL = 10.0                      # VC_CS_SMALL
KCAP = 96                         # VC_CS_KCAP
ATTEMPTS = 64                     # VC_CS_ATTEMPTS
FAIL = -1
M32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: four uint32 words per counter (arrays of one shape, or scalars) under the key (k0, k1)."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(x, shape).copy() for x in c]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def block(seed, idx, draw, mat, stage, attempt):
    idx = np.asarray(idx, dtype=np.uint64)
    c3 = (int(mat) << 16) | (int(stage) << 8) | int(attempt)
    return philox(idx & M32, idx >> np.uint64(32), np.uint64(int(draw)), np.uint64(c3), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def uniform(w, dt):
    return ((w >> np.uint64(9)).astype(dt) + dt(0.5)) * dt(1.0 / 8388608.0)


def _consts(dt):
    if dt is np.float32:
        return dt(0.6931471805599453), dt(1.4426950408889634)
    return dt(math.log(2.0)), dt(1.0 / math.log(2.0))


def _ln(x, dt):
    return _consts(dt)[0] * np.log2(x)


def lfact(k):
    """log(k!) of vc_cs_lfact: float64, whatever the dtype of the rest."""
    dt = np.float64
    x = k + dt(1)
    small = x < dt(8)
    pr = x.copy()
    for j in range(1, 8):
        pr = pr * (x + dt(j))
    corr = np.where(small, np.log(np.where(small, pr, dt(1))), dt(0))
    x = np.where(small, x + dt(8), x)
    inv = dt(1) / x
    inv2 = inv * inv
    ser = inv * (dt(0.083333333333333333) - inv2 * (dt(0.0027777777777777778) - inv2 * dt(0.00079365079365079365)))
    return (((x - dt(0.5)) * np.log(x) - x) + dt(0.91893853320467274)) + (ser - corr)


def gamma(seed, idx, draw, mat, r, dt):
    """gamma(r, 1) variates (Marsaglia-Tsang on polar normals); -1 where the attempts ran out."""
    n = idx.shape[0]
    out = np.full(n, -1.0, dtype=dt)
    boost = r < dt(1)
    rr = np.where(boost, r + dt(1), r)
    d = rr - dt(0.33333333333333333)
    c = dt(1) / np.sqrt(dt(9) * d)
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for a in range(ATTEMPTS):
            if act.size == 0:
                break
            w = block(seed, idx[act], draw, mat, 0, a)
            v1 = dt(2) * uniform(w[0], dt) - dt(1)
            v2 = dt(2) * uniform(w[1], dt) - dt(1)
            s = v1 * v1 + v2 * v2
            ok = s < dt(1)
            x = v1 * np.sqrt((dt(-2) * _ln(s, dt)) / s)
            v = dt(1) + c[act] * x
            ok &= v > dt(0)
            v3 = (v * v) * v
            da = d[act]
            lhs = _ln(uniform(w[2], dt), dt)
            rhs = ((dt(0.5) * (x * x) + da) - da * v3) + da * _ln(np.where(ok, v3, dt(1)), dt)
            ok &= lhs < rhs
            g = da * v3
            ra = r[act]
            g = np.where(boost[act], g * np.exp2(np.log2(uniform(w[3], dt)) / ra), g)
            out[act[ok]] = g[ok]
            act = act[~ok]
    return out


def poisson(seed, idx, draw, mat, lam, dt):
    n = idx.shape[0]
    out = np.full(n, FAIL, dtype=np.int64)
    LN2, LOG2E = _consts(dt)
    with np.errstate(all="ignore"):
        legal = (lam >= dt(0)) & (lam <= dt(MU_MAX))
        # inversion by sequential search
        act = np.nonzero(legal & (lam < dt(SMALL)))[0]
        for a in range(ATTEMPTS):
            if act.size == 0:
                break
            la = lam[act]
            u = uniform(block(seed, idx[act], draw, mat, 1, a)[0], dt)
            p = np.exp2(-(la * LOG2E))
            s = p.copy()
            k = np.zeros(act.size, dtype=np.int64)
            run = np.nonzero(u > s)[0]
            for kk in range(1, KCAP + 1):
                if run.size == 0:
                    break
                p[run] = (p[run] * la[run]) / dt(kk)
                s[run] = s[run] + p[run]
                k[run] = kk
                run = run[u[run] > s[run]]
            done = u <= s
            out[act[done]] = k[done]
            act = act[~done]
        # PTRS
        act = np.nonzero(legal & ~(lam < dt(SMALL)))[0]
        la_all = lam
        for a in range(ATTEMPTS):
            if act.size == 0:
                break
            la = la_all[act]
            slam = np.sqrt(la)
            b = dt(0.931) + dt(2.53) * slam
            al = dt(-0.059) + dt(0.02483) * b
            invalpha = dt(1.1239) + dt(1.1328) / (b - dt(3.4))
            vr = dt(0.9277) - dt(3.6224) / (b - dt(2))
            w = block(seed, idx[act], draw, mat, 1, a)
            U = uniform(w[0], dt) - dt(0.5)
            V = uniform(w[1], dt)
            us = dt(0.5) - np.abs(U)
            kf = np.floor((((dt(2) * al) / us + b) * U + la) + dt(0.43))
            acc = (us >= dt(0.07)) & (V <= vr)
            rej = ~acc & ((kf < dt(0)) | ((us < dt(0.013)) & (V > us)))
            test = ~acc & ~rej
            # the full test in float64 from the dt-rounded V, us, kf, lam and constants (vc_cs_poisson does the same)
            f8 = np.float64
            kt, la8, us8 = np.where(test, kf, dt(0)).astype(f8), la.astype(f8), us.astype(f8)
            lhs = np.log((V.astype(f8) * invalpha.astype(f8)) / (al.astype(f8) / (us8 * us8) + b.astype(f8)))
            rhs = (kt * np.log(la8) - la8) - lfact(kt)
            acc |= test & (lhs <= rhs)
            out[act[acc]] = kf[acc].astype(np.int64)
            act = act[~acc]
    return out


def sample_counts(eta, r, seed, draw, mat, idx, dtype=np.float64):
    """Counts of the documented sampler for natural-log means `eta`, r = 1 / shape_inv per element (None: Poisson) and Philox element
    indices `idx` (uint64), all flat arrays of one length; FAIL (-1) where the device latches its status."""
    dt = np.float32 if dtype in (np.float32, "float32") else np.float64
    eta = np.asarray(eta).astype(dt).reshape(-1)
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    LN2, LOG2E = _consts(dt)
    with np.errstate(all="ignore"):
        mu = np.exp2(eta * LOG2E)
        lam = mu
        bad = np.zeros(eta.shape[0], dtype=bool)
        if r is not None:
            r = np.broadcast_to(np.asarray(r).astype(dt).reshape(-1), eta.shape).copy()
            g = gamma(seed, idx, draw, mat, np.where(r > 0, r, dt(1)), dt)
            bad = ~(r > 0) | (g < 0)
            lam = (g * mu) / r
        k = poisson(seed, idx, draw, mat, np.where(bad, dt(np.nan), lam), dt)
    return k


# ----------------------------------------------------------------------------------------------------------------------------------
# exact moments (share nothing with the sampler) and the 6-standard-error test
# ----------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=2)
def exact_pmf(mu, r):
    """(p, sd): the pmf of Poisson(mu) (r None) or NegativeBinomial(mean mu, shape r) on k = 0 .. far past its mass, from the
    log-pmf of torch.distributions in float64 (a torch tensor), and the distribution's standard deviation."""
    mu = float(mu)
    if r is None:
        sd = math.sqrt(mu)
        dist = torch.distributions.Poisson(torch.tensor(mu, dtype=torch.float64))
    else:
        r = float(r)
        sd = math.sqrt(mu + mu * mu / r)
        dist = torch.distributions.NegativeBinomial(total_count=torch.tensor(r, dtype=torch.float64),
                                                    logits=torch.tensor(math.log(mu) - math.log(r), dtype=torch.float64))
    hi = int(mu + 60.0 * sd + 200)
    if r is not None and r < 1:
        hi = max(hi, int(mu / r * 400) + 1000)
    p = torch.exp(dist.log_prob(torch.arange(0, hi + 1, dtype=torch.float64)))
    # 1e-8: at r = 1e6 the log-pmf's lgamma(k + r) is ~1.3e7 and its float64 rounding 2e-9 of a probability (1e-12 on GRID)
    assert abs(float(p.sum()) - 1.0) < 1e-8, (mu, r, float(p.sum()))
    return p, sd


def exact_moments(mu, r):
    """mean, variance, fourth central moment and P(k = 0) of Poisson(mu) (r None) or NegativeBinomial(mean mu, shape r), from the pmf
    of torch.distributions summed in float64."""
    p, _ = exact_pmf(float(mu), None if r is None else float(r))
    k = torch.arange(0, p.shape[0], dtype=torch.float64)
    m = float((p * k).sum())
    var = float((p * (k - m) ** 2).sum())
    m4 = float((p * (k - m) ** 4).sum())
    return {"mean": m, "var": var, "m4": m4, "p0": float(p[0])}


MIN_EXPECTED = 50.0               # gof_z merges bins until each expects this many samples


def gof_z(k, mu, r, bins=40):
    """Chi-square statistic of the counts `k` against the exact pmf of Poisson(mu) / NegativeBinomial(mu, r), standardised as
    (chi2 - dof) / sqrt(2 dof).  The bins are cut at the exact cdf's j / bins quantiles (bin j = {k : e_(j-1) < k <= e_j}, near-
    equiprobable, both end bins open); cuts that coincide (fewer support points of weight than bins) are dropped and neighbours are
    merged until every bin expects >= MIN_EXPECTED of the len(k) samples; dof = bins left - 1."""
    k = np.asarray(k, dtype=np.int64).reshape(-1)
    n = k.size
    p, _ = exact_pmf(float(mu), None if r is None else float(r))
    cdf = torch.cumsum(p, 0).numpy()
    edges = np.unique(np.searchsorted(cdf, np.arange(1, bins) / bins, side="left"))
    edges = edges[edges < cdf.size - 1]
    upper = np.concatenate([cdf[edges], [1.0]])
    expected = n * np.diff(np.concatenate([[0.0], upper]))
    observed = np.bincount(np.searchsorted(edges, k, side="left"), minlength=edges.size + 1).astype(np.float64)
    # merge left to right until each bin expects enough; a short remainder joins the bin before it
    e_m, o_m, ea, oa = [], [], 0.0, 0.0
    for e, o in zip(expected, observed):
        ea, oa = ea + e, oa + o
        if ea >= MIN_EXPECTED:
            e_m.append(ea), o_m.append(oa)
            ea, oa = 0.0, 0.0
    if ea > 0.0 or oa > 0.0:
        if e_m:
            e_m[-1], o_m[-1] = e_m[-1] + ea, o_m[-1] + oa
        else:
            e_m.append(ea), o_m.append(oa)
    e_m, o_m = np.array(e_m), np.array(o_m)
    dof = e_m.size - 1
    assert dof >= 1, (mu, r, n, "the pmf leaves one bin: nothing to test")
    assert o_m.sum() == n and abs(e_m.sum() - n) < 1e-6 * n
    chi2 = float(((o_m - e_m) ** 2 / e_m).sum())
    return (chi2 - dof) / math.sqrt(2.0 * dof)


def moment_z(k, ex):
    """|sample - exact| / standard error for the sample mean, the sample variance (about the exact mean) and the share of zeros."""
    k = np.asarray(k, dtype=np.float64)
    n = k.size
    z = {"mean": abs(k.mean() - ex["mean"]) / math.sqrt(ex["var"] / n),
         "var": abs(((k - ex["mean"]) ** 2).mean() - ex["var"]) / math.sqrt(max(ex["m4"] - ex["var"] ** 2, 1e-300) / n)}
    p0 = ex["p0"]
    se0 = math.sqrt(p0 * (1.0 - p0) / n)
    z["zero"] = abs((k == 0).mean() - p0) / se0 if se0 > 0 else (0.0 if (k == 0).mean() == p0 else float("inf"))
    return z


# the (mu, r) grid of the sampler tests: both sides of lambda = 10 (Poisson: mu itself; NB: the gamma mixing spreads lambda over both
# branches), r < 1 (boost), r = 1, r > 1, mu << 1 and mu in the hundreds
GRID = [(0.02, None), (3.0, None), (9.5, None), (10.5, None), (40.0, None), (300.0, None),
        (0.05, 0.3), (2.0, 0.5), (12.0, 0.7), (8.0, 1.0), (11.0, 4.0), (60.0, 2.5), (150.0, 0.8), (400.0, 10.0), (9.9, 50.0), (25.0, 200.0)]


# rates up to the documented VC_CS_MU_MAX = 2^20.  The Poisson cells are the sensitive probe of PTRS's full test (both sides of 2^16,
# the last just under 2^20); in the NB cells the gamma's own spread hides most of what PTRS does wrong, they hold the mixing to the
# pmf at large rates (tests/test_ppc_cpu.py checks that the mixed rates stay inside the range)
LARGE_GRID = [(1.0e3, None), (1.0e4, None), (6.5e4, None), (1.0e5, None), (5.0e5, None), (1.0e6, None),
              (1.0e4, 2.0), (3.0e4, 50.0), (2.0e5, 20.0), (2.0e5, 2000.0)]


def handed_rate(mu):
    """exp(float64(float32(log mu))): the rate a sampler handed eta = float32(log mu) is asked for."""
    return math.exp(float(np.float32(math.log(mu))))


def device_r(r):
    """The float32 r = 1 / shape_inv the device forms when it is handed shape_inv = float32(1 / r)."""
    return np.float32(1.0) / (np.float32(1.0) / np.float32(r))


def grid_inputs(n_per_cell, grid=None, as_device=False):
    """eta (float32), r (float32 or nan for Poisson; device_r of the grid's r if as_device) of the grid laid out cell after cell."""
    grid = GRID if grid is None else grid
    eta = np.concatenate([np.full(n_per_cell, np.float32(math.log(mu)), dtype=np.float32) for mu, _ in grid])
    r = np.concatenate([np.full(n_per_cell, np.nan if rr is None else (device_r(rr) if as_device else rr), dtype=np.float32) for _, rr in grid])
    return eta, r


def sample_grid(n_per_cell, seed, draw, dtype, grid=None, as_device=False):
    """The restated sampler over a grid (GRID unless given): Poisson cells as matrix 0, NB cells as matrix 1, element index =
    position in the layout."""
    eta, r = grid_inputs(n_per_cell, grid, as_device)
    idx = np.arange(eta.size, dtype=np.uint64)
    out = np.empty(eta.size, dtype=np.int64)
    pois = np.isnan(r)
    out[pois] = sample_counts(eta[pois], None, seed, draw, 0, idx[pois], dtype)
    out[~pois] = sample_counts(eta[~pois], r[~pois], seed, draw, 1, idx[~pois], dtype)
    return out


def cell_z(k, mu, r):
    """moment_z and gof_z of one cell's counts against the exact distribution at (mu, r): {"mean", "var", "zero", "gof"}."""
    r = None if r is None else float(r)
    z = moment_z(k, exact_moments(mu, r))
    z["gof"] = gof_z(k, mu, r)
    return z


def cap(n_diff32, n):
    """Elements the device may differ from the float64 checker in: SAFETY x the float32 restatement's own count, at least FLOOR."""
    return max(FLOOR, int(math.ceil(SAFETY * n_diff32)))


# ----------------------------------------------------------------------------------------------------------------------------------
# the engine path: dense eta of a fixture's draws, replicates, statistics, p-values
# ----------------------------------------------------------------------------------------------------------------------------------
def dense_eta(z, dtype=torch.float64):
    """{matrix: eta (D, Ng, Nc)} of a fixture (natural-log mean of every element under every draw) and r (D, Ng, 1) or None."""
    p = PC.problem_of(z, dtype)
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
    r = (1.0 / dr["shape_inv"])[:, :, None] if p["noise"] == "NegativeBinomial" else None
    return out, r


def element_index(Ng, Nc, cell_offset=0):
    """Philox element index of (gene g, GLOBAL cell c): g << 32 | c, shape (Ng, Nc)."""
    return (np.arange(Ng, dtype=np.uint64)[:, None] << np.uint64(32)) | (np.arange(Nc, dtype=np.uint64)[None, :] + np.uint64(cell_offset))


def replicates(z, seed, dtype=np.float64, cell_offset=0, draw0=0):
    """{matrix: (D, Ng, Nc) int64} replicated counts of a fixture's draws under the documented sampler in `dtype` arithmetic (eta is
    formed in the same precision)."""
    tdt = torch.float32 if dtype in (np.float32, "float32") else torch.float64
    eta, r = dense_eta(z, tdt)
    out = {}
    for mi, m in enumerate(eta):
        e = eta[m].numpy()
        D, Ng, Nc = e.shape
        idx = element_index(Ng, Nc, cell_offset).reshape(-1)
        rep = np.empty((D, Ng, Nc), dtype=np.int64)
        for d in range(D):
            rr = None if r is None else np.broadcast_to(r[d].numpy(), (Ng, Nc)).reshape(-1)
            rep[d] = sample_counts(e[d].reshape(-1), rr, seed, draw0 + d, mi, idx, dtype).reshape(Ng, Nc)
        out[m] = rep
    return out


def mixed_rates(z, seed, cell_offset=0, draw0=0):
    """{matrix: (D, Ng, Nc) float64} the Poisson rate of every element of a fixture's draws: exp(eta), for the negative binomial
    times gamma / r with the float64 restatement's gamma variate of that element (which does not depend on eta)."""
    eta, r = dense_eta(z, torch.float64)
    out = {}
    for mi, m in enumerate(eta):
        lam = np.exp(eta[m].numpy())
        D, Ng, Nc = lam.shape
        idx = element_index(Ng, Nc, cell_offset).reshape(-1)
        for d in range(D if r is not None else 0):
            rr = np.broadcast_to(r[d].numpy(), (Ng, Nc)).reshape(-1).copy()
            lam[d] *= (gamma(seed, idx, draw0 + d, mi, rr, np.float64) / rr).reshape(Ng, Nc)
        out[m] = lam
    return out


def rep_stats(rep):
    """Per-draw tables of replicates (D, Ng, Nc): gene (D, 4, Ng) = sum k, sum k^2, #{k = 0}, max k over cells; cell (D, Nc) = sum over genes."""
    rep = np.asarray(rep, dtype=np.int64)
    gene = np.stack([rep.sum(2), (rep * rep).sum(2), (rep == 0).sum(2), rep.max(2)], axis=1)
    return gene, rep.sum(1)


def obs_stats(k):
    """The same five statistics of observed counts (Ng, Nc), float64."""
    k = np.asarray(k, dtype=np.float64)
    return np.stack([k.sum(1), (k * k).sum(1), (k == 0).sum(1).astype(np.float64), k.max(1)]), k.sum(0)


def derived(gene, n_cells):
    """T in (mean, variance, zero fraction, max) per gene from a (..., 4, Ng) table over n_cells cells, float64: (..., 4, Ng)."""
    g = np.asarray(gene, dtype=np.float64)
    mean = g[..., 0, :] / n_cells
    var = g[..., 1, :] / n_cells - mean * mean
    return np.stack([mean, var, g[..., 2, :] / n_cells, g[..., 3, :]], axis=-2)


def p_values(t_rep, t_obs):
    """p_ge, p_gt, p_mid over the leading (draw) axis."""
    ge = (t_rep >= t_obs).mean(0)
    gt = (t_rep > t_obs).mean(0)
    return ge, gt, 0.5 * (ge + gt)
