"""Checker of the joint per-gene fit (velocycle_amd.gene_joint.gene_joint / velocity_map_joint / vc_gene_joint), written from the
formulas.  Per gene and cell, with theta = (nu [K], x = log gamma, y = log beta), b = [1, sin phi, cos phi, ...], db its phi-derivative
taken from the same rows (db_0 = 0, db_{2h-1} = h b_{2h}, db_{2h} = -h b_{2h-1}), W the angular speed's design:

    etaS = nu . b + logm,   d = nu . db,   om = nuw . W,   z = om d + e^x,   a = [z > 0],   zp = a z + 1e-5
    etaU = etaS - y + ln zp,   muS = e^etaS,   muU = e^etaU
    f = L_S + L_U - (theta - m)' Lambda (theta - m) / 2          (Poisson | NegativeBinomial at one r per gene for both layers)
    s = a om / zp,   p = a e^x / zp,   q = a d / zp,   u = (s db, p, 0),   gS = (b, 0, 0),   gU = (b + s db, p, -1)
    gradient   G = sum resS gS + resU gU - Lambda (theta - m)
    observed   O = sum woS gS gS' + woU gU gU' + resU u u' - [sum resU p]_xx + Lambda
    Fisher     F = sum wS gS gS' + wU gU gU' + Lambda
    N_i = sum (woS^2 + resS^2) gS_i^2 + (woU^2 + resU^2) gU_i^2
    score_i = sum resU q W_i;   profile information  I_ww - I_wt (I_tt + Lambda)^-1 I_tw,  I over (q W, gU) for U plus gS for S

`point64` is these lines in float64 from float64 tables; `solve64` the hybrid Newton iteration (A = O where its Cholesky factorisation
succeeds, else F; step halved while f drops) run to dec <= 1e-24 max(1, |f|); `map64` the outer Newton iteration over nuw.

`point32` restates the device kernel's contract: tables rounded to float32, etaS, d, om, z and etaS - y float64, e^etaS and e^(etaS - y)
rounded once to float32 (the latter multiplied by zp in float32), residuals, weights, the NB logarithm and ln zp float32, float64 sums
over reversed cells; `solve32` and `map32` run the contract's rules on it (tol, the rounding rule, the halving allowance, the box, the
fall-back of a start outside it, the exclusion of genes after the first round).  The restatement's own distance from the reference sets
every bar (SAFETY x its worst over the GPU cases), never the code under test.

Problems are `tests.gene_kinetics_checker.simulate`'s, with S drawn from the problem's own nu (Poisson, or Gamma-Poisson at its r);
seeds are fixed and chosen such that the reference alone stays kink-free (min z >= MIN_Z at every point it evaluates, refused trials
included) and converges."""
import math
from functools import lru_cache

import numpy as np
from scipy.special import gammaln

from tests.gene_glm_checker import EPS32, SAFETY, _sum_other_order, logp64
from tests.gene_kinetics_checker import (FLOOR, HALVINGS, MIN_Z, NUW_BY_NW, NUW_PRIOR_STD, OUTER_HALVINGS, PRIOR, TOL, TOL_OUTER, MAX_ROUNDS,
                                         basis64, dbasis64, design64, directions, nuw_prior, simulate, sym_distance)

EPS64 = float(np.finfo(np.float64).eps)
CONVERGED, ROUNDING, MAX_ITER, UNBOUNDED, NO_DATA, EVALUATED = range(6)
INTERIOR = (CONVERGED, ROUNDING)
NU_BOUND, XY_BOUND = 50.0, 30.0
MAX_ITER_DEFAULT = 40
NU_PRIOR = (0.0, 3.0)                      # Cycle.trivial_prior's default Normal(0, 3)
S_SEED = 77                                # the stream the spliced counts are drawn from
NB, PO = "NegativeBinomial", "Poisson"
__all__ = ["dbasis64", "design64", "directions", "NUW_PRIOR_STD"]          # re-exported for the tests


def prior_of(K, nu_prior=NU_PRIOR, kin=PRIOR):
    """(means, precisions) of theta, float64 [K + 2]."""
    m = np.array([nu_prior[0]] * K + [kin[0], kin[2]], dtype=np.float64)
    s = np.array([nu_prior[1]] * K + [kin[1], kin[3]], dtype=np.float64)
    return m, 1.0 / s ** 2


def bounds(K):
    return np.array([NU_BOUND] * K + [XY_BOUND] * 2)


def db_from_basis(B):
    """The phi-derivative of the basis from its own rows (what the kernel does: no second table)."""
    dB = np.zeros_like(B)
    for h in range(1, (B.shape[0] - 1) // 2 + 1):
        dB[2 * h - 1], dB[2 * h] = h * B[2 * h], -h * B[2 * h - 1]
    return dB


# ---------------------------------------------------------------------------------------------------------------- problems
def with_spliced(p, seed):
    """The kinetics checker's problem with S [Nc, Ng] drawn from its own nu."""
    rng = np.random.default_rng([S_SEED, seed])
    B, logm = basis64(p["phis"], p["H"]), np.log(p["n"])
    S = np.zeros_like(p["U"])
    for g in range(S.shape[1]):
        mu = np.exp(p["nu"][g] @ B + logm)
        lam = mu if p["r"] is None else rng.gamma(p["r"][g], mu / p["r"][g])
        S[:, g] = rng.poisson(lam)
    S[0, S.sum(0) == 0] = 1.0
    return dict(p, S=S)


# name: (seed, Nc, Ng, H, noise, extra keywords of simulate)
SHAPES = [(1, 1, 1, PO), (63, 2, 2, NB), (64, 3, 1, NB), (65, 4, 2, PO), (255, 5, 1, PO), (256, 1, 2, NB), (257, 5, 1, NB), (257, 5, 2, PO),
          (1025, 3, 1, PO), (1025, 3, 2, NB)]
SEEDS = {}                                 # filled below: case name -> seed (chosen on the CPU, see the module's docstring)
RECOVERY_SHAPES = [(257, 5, 1, PO), (1025, 6, 2, NB), (65, 4, 1, NB), (64, 5, 2, PO), (3000, 8, 1, NB)]     # the prototype's
EVALUATE_CASE = "shape_257_5_1_NegativeBinomial"
EVALUATE_AT = [None, (0.0, 0.0, 2.0), (0.02, -0.5, 1.0), (-0.03, 0.6, 3.0), (0.0, -2.0, 2.5)]
"""(shift of every harmonic from the truth, x, y); None: the kernel's own start; the last one clamps cells"""
SCORE_CASES = ["score_257_5_1", "score_257_5_2", "score_257_5_3", "score_1025_3_1", "score_1025_3_2", "score_1025_3_3"]
OUTER_CASES = ["outer_3000_40", "outer_1500_30"]
LARGE_CASES = ["large_u16", "large_f32"]
FIT_CASES = [f"shape_{Nc}_{Ng}_{H}_{noise}" for Nc, Ng, H, noise in SHAPES] + LARGE_CASES
# chosen on the CPU, the first of a run of seeds for which the reference alone is kink-free at EVERY point it evaluates (refused
# trials included), converges in every gene, and the restatement stops within a step of it (large cases: counts in their range)
SEEDS.update({"shape_1_1_1_Poisson": 1000, "shape_63_2_2_NegativeBinomial": 1000, "shape_64_3_1_NegativeBinomial": 1000,
              "shape_65_4_2_Poisson": 1000, "shape_255_5_1_Poisson": 1044, "shape_256_1_2_NegativeBinomial": 1001,
              "shape_257_5_1_NegativeBinomial": 1005, "shape_257_5_2_Poisson": 1007, "shape_1025_3_1_Poisson": 1004,
              "shape_1025_3_2_NegativeBinomial": 1004, "large_u16": 2007, "large_f32": 3000, "score_257_5_1": 4011, "score_257_5_2": 5008,
              "score_257_5_3": 6093, "score_1025_3_1": 7007, "score_1025_3_2": 8006, "score_1025_3_3": 9002, "recovery_0": 10026,
              "recovery_1": 11017, "recovery_2": 12000, "recovery_3": 13000, "recovery_4": 14004})
SEEDS.update({"outer_3000_40": 20000, "outer_1500_30": 21003, "kink_a": 50, "far": 150})


@lru_cache(maxsize=None)
def cases():
    out = {}
    for Nc, Ng, H, noise in SHAPES:
        name = f"shape_{Nc}_{Ng}_{H}_{noise}"
        out[name] = with_spliced(simulate(SEEDS[name], Nc, Ng, H, noise, [0.4]), SEEDS[name])
    for i, name in enumerate(SCORE_CASES):
        _, Nc, Ng, NW = name.split("_")
        nuw, Hw, Nx = NUW_BY_NW[int(NW)]
        out[name] = with_spliced(simulate(SEEDS[name], int(Nc), int(Ng), 1 + i % 2, NB if i % 2 else PO, np.atleast_1d(nuw), Hw=Hw, Nx=Nx),
                                 SEEDS[name])
    out["outer_3000_40"] = with_spliced(simulate(SEEDS["outer_3000_40"], 3000, 40, 1, NB, [0.4]), SEEDS["outer_3000_40"])
    out["outer_1500_30"] = with_spliced(simulate(SEEDS["outer_1500_30"], 1500, 30, 1, PO, [0.45, 0.3], Nx=2, level=(4.0, 5.5)),
                                        SEEDS["outer_1500_30"])
    out["kink_a"] = with_spliced(simulate(SEEDS["kink_a"], 1025, 4, 1, PO, [1.5], gamma_range=(-1.0, -0.6), amp_scale=0.9), 50)
    out["far"] = with_spliced(simulate(SEEDS["far"], 257, 3, 1, PO, [0.4]), 150)
    out["large_u16"] = with_spliced(simulate(SEEDS["large_u16"], 257, 2, 1, PO, [0.4], level=(4.0, 4.5), big=2500.0), SEEDS["large_u16"])
    out["large_f32"] = with_spliced(simulate(SEEDS["large_f32"], 257, 2, 1, NB, [0.4], level=(4.0, 4.5), big=2600.0), SEEDS["large_f32"])
    return out


@lru_cache(maxsize=None)
def recovery_cases():
    """The shapes of the prototype the issue reports (every parameter within 4 standard errors of the simulated truth)."""
    out = {}
    for i, (Nc, Ng, H, noise) in enumerate(RECOVERY_SHAPES):
        kw = dict(level=(4.5, 5.5), gamma_range=(0.2, 0.5)) if (Nc, Ng) == (64, 5) else {}
        out[f"recovery_{i}"] = with_spliced(simulate(SEEDS[f"recovery_{i}"], Nc, Ng, H, noise, [0.4], **kw), SEEDS[f"recovery_{i}"])
    return out


def gene_inputs(p, g):
    """kS, kU, B, logm, r of gene g."""
    return p["S"][:, g], p["U"][:, g], basis64(p["phis"], p["H"]), np.log(p["n"]), (p["r"][g] if p["r"] is not None else None)


def truth(p, g):
    return np.concatenate([p["nu"][g], [p["x"][g], p["y"][g]]])


# ---------------------------------------------------------------------------------------------------------------- one point
def _chol_ok(M):
    if not np.isfinite(M).all():
        return False
    try:
        np.linalg.cholesky(M)
        return True
    except np.linalg.LinAlgError:
        return False


def _finish(th, B, W, a, ex, zp, d, om, lS, lU, L_S, L_U, A, prior, other_order):
    """From the per-cell pieces (lS, lU = (res, w, wo) of each layer) to everything the iteration and the outputs need."""
    S = _sum_other_order if other_order else (lambda v: np.asarray(v, dtype=np.float64).sum(-1))
    K, Nc = B.shape
    D = K + 2
    pm, pp = prior
    dB = db_from_basis(B)
    p, s, q = np.where(a, ex / zp, 0.0), np.where(a, om / zp, 0.0), np.where(a, d / zp, 0.0)
    gS = np.concatenate([B, np.zeros((2, Nc))])
    gU = np.concatenate([B + s * dB, p[None], -np.ones((1, Nc))])
    u = np.concatenate([s * dB, p[None], np.zeros((1, Nc))])
    (rS, wS, oS), (rU, wU, oU) = lS, lU
    G = S(rS * gS) + S(rU * gU) - pp * (th - pm)
    outer = lambda v, wt: S(wt * v[:, None, :] * v[None, :, :])                     # noqa: E731
    O = outer(gS, oS) + outer(gU, oU) + outer(u, rU) + np.diag(pp)
    O[K, K] -= S(rU * p)
    F = outer(gS, wS) + outer(gU, wU) + np.diag(pp)
    observed = _chol_ok(O)
    M = O if observed else F
    inv = np.linalg.inv(M)
    step = inv @ G
    pen = 0.5 * float((pp * (th - pm) ** 2).sum())
    qW = q[None, :] * W
    NW = W.shape[0]
    Iww = np.array([[S(wU * qW[i] * qW[j]) for j in range(NW)] for i in range(NW)]).reshape(NW, NW)
    Iwt = np.array([S(wU * qW[i] * gU) for i in range(NW)]).reshape(NW, D)
    return dict(th=th, L_S=L_S, L_U=L_U, L=L_S + L_U, A=A, f=L_S + L_U - pen, G=G, M=M, O=O, F=F, observed=observed, inv=inv, step=step,
                dec=float(G @ step), fisher_step=np.linalg.solve(F, G),
                N=S((oS * oS + rS * rS) * gS * gS) + S((oU * oU + rU * rU) * gU * gU), n_clamped=int((~a).sum()),
                score=np.array([S(rU * qW[i]) for i in range(NW)]), info=Iww - Iwt @ np.linalg.inv(F) @ Iwt.T,
                score_unit=4 * EPS32 * np.sqrt(np.array([S((wU * wU + rU * rU) * qW[i] ** 2) for i in range(NW)])),
                minz=float(np.where(a, zp - FLOOR, -1.0).min()))


def _lik64(k, eta, noisemodel, r):
    mu = np.exp(eta)
    if noisemodel == PO:
        res, w, wo = k - mu, mu, mu
        parts = np.abs(k * eta) + gammaln(k + 1) + mu
    else:
        res, w, wo = (k - mu) * r / (r + mu), mu * r / (r + mu), mu * r * (k + r) / (r + mu) ** 2
        parts = np.abs(k * eta) + gammaln(k + 1) + gammaln(k + r) + abs(gammaln(r)) + abs(r * math.log(r)) + (k + r) * np.abs(np.log(r + mu))
    return (res, w, wo), logp64(k, eta, noisemodel, r), parts


def point64(th, kS, kU, B, logm, W, nuw, noisemodel, r=None, prior=None):
    """The reference at theta.  L_S, L_U are the FULL log-likelihoods; abs_S, abs_U = sum_c |log p_c|."""
    th = np.asarray(th, dtype=np.float64)
    K = B.shape[0]
    prior = prior_of(K) if prior is None else prior
    nu, x, y = th[:K], th[K], th[K + 1]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d, om, ex = nu @ db_from_basis(B), nuw @ W, math.exp(x)
        z = om * d + ex
        a = z > 0
        zp = np.where(a, z, 0.0) + FLOOR
        etaS = nu @ B + logm
        etaU = etaS - y + np.log(zp)
        lS, lpS, partsS = _lik64(kS, etaS, noisemodel, r)
        lU, lpU, partsU = _lik64(kU, etaU, noisemodel, r)
        out = _finish(th, B, W, a, ex, zp, d, om, lS, lU, float(lpS.sum()), float(lpU.sum()), float(partsS.sum() + partsU.sum()), prior, False)
        out["abs_S"], out["abs_U"] = float(np.abs(lpS).sum()), float(np.abs(lpU).sum())
    return out


def constants64(k, noisemodel, r):
    """The part of a layer's log-likelihood the kernel's objective leaves out (its NB objective holds r ln r)."""
    if noisemodel == PO:
        return float(-gammaln(k + 1).sum())
    return float((gammaln(k + r) - gammaln(r) - gammaln(k + 1)).sum())


def _lik32(k32, mu, eta, noisemodel, r32):
    """gene_lik: float32 residual and weights, float64 terms and magnitudes."""
    f32 = np.float32
    kd = k32.astype(np.float64)
    if noisemodel == PO:
        res, w, wo = k32 - mu, mu, mu
        terms = kd * eta - mu.astype(np.float64)
        mag = np.abs(kd * eta) + mu.astype(np.float64)
    else:
        s = r32 + mu
        pr = r32 / s
        res, w, wo = (k32 - mu) * pr, mu * pr, (mu / s) * pr * (k32 + r32)
        big = mu >= r32
        xx = np.where(big, r32, mu) / np.where(big, mu, r32)
        lg = np.log(f32(1) + xx.astype(f32)).astype(np.float64)
        lnr = math.log(float(r32))
        e = eta - lnr
        terms = kd * np.where(big, -lg, e - lg) - float(r32) * np.where(big, e + lg, lg)
        mag = (kd + float(r32)) * np.abs(np.where(big, eta, lnr) + lg) + np.abs(kd * eta)
    return tuple(v.astype(np.float64) for v in (res, w, wo)), terms, mag


def point32(th, kS, kU, B, logm, W, nuw, noisemodel, r=None, prior=None):
    """The kernel's contract at theta.  L_S, L_U are the full log-likelihoods (the float64 constants added), A the kernel's sum |terms|."""
    f32 = np.float32
    th = np.asarray(th, dtype=np.float64)
    K = B.shape[0]
    prior = prior_of(K) if prior is None else prior
    nu, x, y = th[:K], th[K], th[K + 1]
    B32, logm32, W32 = B.astype(f32).astype(np.float64), logm.astype(f32).astype(np.float64), W.astype(f32).astype(np.float64)
    r32 = f32(r) if noisemodel == NB else None
    rc = float(r32) if r32 is not None else None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d, om, ex = nu @ db_from_basis(B32), nuw @ W32, math.exp(x)
        z = om * d + ex
        a = z > 0
        zp = np.where(a, z + FLOOR, FLOOR)
        etaS = nu @ B32 + logm32
        e0 = etaS - y
        zpf = zp.astype(f32)
        muS = np.exp(etaS).astype(f32)
        muU = np.exp(e0).astype(f32) * zpf
        etaU = e0 + np.log(zpf).astype(np.float64)
        lS, tS, mS = _lik32(kS.astype(f32), muS, etaS, noisemodel, r32)
        lU, tU, mU = _lik32(kU.astype(f32), muU, etaU, noisemodel, r32)
        return _finish(th, B32, W32, a, ex, zp, d, om, lS, lU, float(_sum_other_order(tS)) + constants64(kS, noisemodel, rc),
                       float(_sum_other_order(tU)) + constants64(kU, noisemodel, rc), float(_sum_other_order(mS + mU)), prior, True)


# ---------------------------------------------------------------------------------------------------------------- inner iteration
def start_theta(kS, kU, B, logm, W, nuw, prior):
    """The default start: nu_0 = ln(sum k_S / sum e^logm), harmonics at their prior means, x = mu_gamma, y = ln(sum e^etaS zp / sum k_U)."""
    K = B.shape[0]
    th = prior[0].copy()
    th[0] = math.log(kS.sum() / np.exp(logm).sum())
    z = (nuw @ W) * (th[:K] @ db_from_basis(B)) + math.exp(th[K])
    zp = np.where(z > 0, z, 0.0) + FLOOR
    th[K + 1] = math.log((np.exp(th[:K] @ B + logm) * zp).sum() / kU.sum())
    return np.clip(th, -bounds(K), bounds(K))


def _inside(th, K):
    return bool((np.abs(th) <= bounds(K)).all())


def _iterate(point, th, tol, max_iter, eps, rounding_rule):
    """The contract's iteration on `point(theta)`.  tol: a number, or a function of the point (the reference's relative tolerance).
    `minz_path` is the least z over every point evaluated (refused trials included), `first_tol` the steps taken when dec first fell
    to TOL."""
    K = len(th) - 2
    e = point(th)
    minz = e["minz"]
    first = 0 if e["dec"] <= TOL else None
    if max_iter == 0:
        return dict(e, iterations=0, status=EVALUATED, fisher_retries=0, minz_path=minz, first_tol=first)
    steps, halvings, status, retries = 0, HALVINGS, MAX_ITER, 0
    while True:
        if not np.isfinite(e["dec"]):
            break
        if e["dec"] <= (tol(e) if callable(tol) else tol):
            status = CONVERGED
            break
        if rounding_rule and (np.abs(e["G"]) <= 4 * EPS32 * np.sqrt(e["N"])).all():
            status = ROUNDING
            break
        if steps >= max_iter:
            break
        t, moved, step = 1.0, False, e["step"]
        if e["observed"] and not _inside(e["th"] + step, K):
            step = e["fisher_step"]                # a barely positive definite observed matrix: the Fisher step before giving up
            retries += 1
        if not _inside(e["th"] + step, K):
            status = UNBOUNDED
            break
        while True:
            trial = point(e["th"] + t * step)
            minz = min(minz, trial["minz"])
            if trial["f"] >= e["f"] - 8 * eps * max(trial["A"], e["A"]):
                e, moved = trial, True
                break
            if halvings == 0:
                break
            halvings -= 1
            t *= 0.5
        if not moved:
            break
        steps += 1
        if first is None and e["dec"] <= TOL:
            first = steps
    return dict(e, iterations=steps, status=status, fisher_retries=retries, minz_path=minz, first_tol=first)


def _start(start, default, K):
    if start is None:
        return default
    start = np.asarray(start, dtype=np.float64)
    return start if np.isfinite(start).all() and _inside(start, K) else default


def solve64(kS, kU, B, logm, W, nuw, noisemodel, r=None, prior=None, start=None, max_iter=80):
    prior = prior_of(B.shape[0]) if prior is None else prior
    pt = lambda th: point64(th, kS, kU, B, logm, W, nuw, noisemodel, r, prior)         # noqa: E731
    th = _start(start, start_theta(kS, kU, B, logm, W, nuw, prior), B.shape[0])
    return _iterate(pt, th, lambda e: 1e-24 * max(1.0, abs(e["f"])), max_iter, EPS64, False)


def solve32(kS, kU, B, logm, W, nuw, noisemodel, r=None, prior=None, start=None, tol=TOL, max_iter=MAX_ITER_DEFAULT):
    prior = prior_of(B.shape[0]) if prior is None else prior
    pt = lambda th: point32(th, kS, kU, B, logm, W, nuw, noisemodel, r, prior)         # noqa: E731
    f32 = lambda v: v.astype(np.float32).astype(np.float64)                            # noqa: E731
    th = _start(start, start_theta(kS, kU, f32(B), f32(logm), f32(W), nuw, prior), B.shape[0])
    return _iterate(pt, th, tol, max_iter, EPS32, True)


def _solved(p, nuw=None):
    v = p["nuw"] if nuw is None else np.asarray(nuw, dtype=np.float64)
    out = []
    for g in range(p["U"].shape[1]):
        kS, kU, B, logm, r = gene_inputs(p, g)
        out.append((solve64(kS, kU, B, logm, p["W"], v, p["noisemodel"], r), solve32(kS, kU, B, logm, p["W"], v, p["noisemodel"], r)))
    return out


@lru_cache(maxsize=None)
def solved(name):
    """Per gene (reference, restatement) of a case at its own nuw."""
    return _solved(cases()[name])


def assert_kink_free(name, fits):
    """A tolerance-bearing case: min z >= MIN_Z at every point the reference visits, and >= 90 % of its genes CONVERGED there."""
    assert min(f64["minz_path"] for f64, _ in fits) >= MIN_Z, (name, [f64["minz_path"] for f64, _ in fits])
    assert np.mean([f64["status"] == CONVERGED for f64, _ in fits]) >= 0.9, (name, [f64["status"] for f64, _ in fits])


# ---------------------------------------------------------------------------------------------------------------- outer iteration
def _outer(p, solve, ok, tol_outer, max_rounds, allowance, nuw0=None, trace=None):
    Ng = p["U"].shape[1]
    pm, pp = nuw_prior(p["Nx"], p["Hw"])
    genes = [gene_inputs(p, g) for g in range(Ng)]

    def evaluate(v, starts, inc):
        fits = [solve(kS, kU, B, logm, p["W"], v, p["noisemodel"], r, start=None if starts is None else starts[g])
                for g, (kS, kU, B, logm, r) in enumerate(genes)]
        good = np.array([ok(f) for f in fits])
        inc = good if inc is None else inc
        d = v - pm
        sel = [f for f, i in zip(fits, inc) if i]
        if trace is not None:
            trace.append((v.copy(), min(f["minz_path"] for f in sel)))
        return dict(fits=fits, inc=inc, failed=bool((inc & ~good).any()), F=sum(f["f"] for f in sel) - 0.5 * (pp * d * d).sum(),
                    allow=allowance * sum(abs(f["L"]) for f in sel), G=sum(f["score"] for f in sel) - pp * d,
                    J=sum(f["info"] for f in sel) + np.diag(pp))

    v = pm.copy() if nuw0 is None else np.asarray(nuw0, dtype=np.float64)
    cur = evaluate(v, None, None)
    inc = cur["inc"]
    status, rounds, dec = "MAX_ROUNDS", 0, float("nan")
    while inc.any():
        step = np.linalg.solve(cur["J"], cur["G"])
        dec = float(cur["G"] @ step)
        if dec <= tol_outer:
            status = "CONVERGED"
            break
        if rounds >= max_rounds:
            break
        t, moved = 1.0, False
        for _ in range(OUTER_HALVINGS + 1):
            trial = evaluate(v + t * step, [f["th"] for f in cur["fits"]], inc)
            if trial["failed"]:
                status = "GENE_FAILED"
                break
            if trial["F"] >= cur["F"] - max(cur["allow"], trial["allow"]):
                v, cur, moved = v + t * step, trial, True
                break
            t *= 0.5
        else:
            status = "STALLED"
        if not moved:
            break
        rounds += 1
    cov = np.linalg.inv(cur["J"])
    return dict(nuw=v, cov=cov, J=cur["J"], std=np.sqrt(np.diag(cov)), F=cur["F"], G=cur["G"], dec=dec, rounds=rounds, status=status,
                fits=cur["fits"], included=inc, n_excluded=int((~inc).sum()))


def map64(p, nuw0=None, trace=None):
    return _outer(p, solve64, lambda f: f["status"] == CONVERGED, 1e-14, 60, 8 * EPS64, nuw0, trace)


def map32(p, nuw0=None):
    return _outer(p, solve32, lambda f: f["status"] in INTERIOR, TOL_OUTER, MAX_ROUNDS, 8 * EPS32, nuw0)


def profile64(p, v, genes=None, starts=None):
    """F(v) of the reference and its envelope score and information; every gene solved from the default start, or from starts[g]
    (F does not depend on the start: a start near the optimum keeps a large case's paths away from the kink)."""
    pm, pp = nuw_prior(p["Nx"], p["Hw"])
    v = np.asarray(v, dtype=np.float64)
    fits = []
    for g in (range(p["U"].shape[1]) if genes is None else genes):
        kS, kU, B, logm, r = gene_inputs(p, g)
        fits.append(solve64(kS, kU, B, logm, p["W"], v, p["noisemodel"], r, start=None if starts is None else starts[g]))
    assert all(f["status"] == CONVERGED for f in fits)
    d = v - pm
    return dict(F=sum(f["f"] for f in fits) - 0.5 * (pp * d * d).sum(), G=sum(f["score"] for f in fits) - pp * d,
                J=sum(f["info"] for f in fits) + np.diag(pp), minz=min(f["minz_path"] for f in fits))


@lru_cache(maxsize=None)
def outer_solved(name):
    """(reference, restatement, the reference's trace [(nuw, min z)]) of an outer case."""
    trace = []
    p = cases()[name]
    return map64(p, trace=trace), map32(p), trace


# ---------------------------------------------------------------------------------------------------------------- distances and bars
def theta_distance(th, ref):
    """sqrt(delta' A64 delta): the distance in the reference's standard errors."""
    d = np.asarray(th, dtype=np.float64) - ref["th"]
    return float(math.sqrt(max(d @ ref["M"] @ d, 0.0)))


def loglik_distance(L, ref, layer):
    return abs(L - ref["L_" + layer]) / (EPS32 * ref["abs_" + layer])


def dec_distance(dec, ref):
    """|dec - dec_ref| in units of what the gradient's float32 noise (4 eps32 sqrt(N_i)) does to it."""
    nz = 4 * EPS32 * np.sqrt(ref["N"])
    n2 = float(nz @ np.abs(ref["inv"]) @ nz)
    return abs(dec - ref["dec"]) / (2 * math.sqrt(max(ref["dec"], 0.0) * n2) + n2)


def score_distance(score, ref):
    return float((np.abs(score - ref["score"]) / ref["score_unit"]).max())


def evaluate_points(p, g):
    """The theta of EVALUATE_AT for gene g."""
    kS, kU, B, logm, r = gene_inputs(p, g)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)                            # noqa: E731
    K = B.shape[0]
    own = start_theta(kS, kU, f32(B), f32(logm), f32(p["W"]), p["nuw"], prior_of(K))
    out = []
    for at in EVALUATE_AT:
        if at is None:
            out.append(own)
        else:
            nu = p["nu"][g].copy()
            nu[1:] += at[0]
            out.append(np.concatenate([nu, at[1:]]))
    return out


@lru_cache(maxsize=None)
def evaluated():
    """{(i, g): (reference, restatement)} at EVALUATE_AT[i] of EVALUATE_CASE."""
    p = cases()[EVALUATE_CASE]
    out = {}
    for g in range(p["U"].shape[1]):
        kS, kU, B, logm, r = gene_inputs(p, g)
        for i, th in enumerate(evaluate_points(p, g)):
            out[(i, g)] = (point64(th, kS, kU, B, logm, p["W"], p["nuw"], p["noisemodel"], r),
                           point32(th, kS, kU, B, logm, p["W"], p["nuw"], p["noisemodel"], r))
    return out


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst distance from the reference over the GPU cases, per asserted figure; `steps` is the
    restatement's worst number of steps per gene (not multiplied)."""
    w = dict(theta=0.0, cov=0.0, loglik=0.0, loglik_large=0.0, ev_loglik=0.0, ev_dec=0.0, score=0.0, info=0.0, nuw=0.0, std=0.0)
    steps = 0
    for name in FIT_CASES + SCORE_CASES:
        fits = solved(name)
        assert_kink_free(name, fits)
        for f64, f32 in fits:
            if f64["status"] != CONVERGED:
                continue
            assert f32["status"] in INTERIOR, (name, f32["status"])
            steps = max(steps, f32["iterations"])
            w["theta"] = max(w["theta"], theta_distance(f32["th"], f64))
            w["cov"] = max(w["cov"], sym_distance(f32["inv"], f64["inv"]))
            key = "loglik_large" if name in LARGE_CASES else "loglik"      # at counts of 1e4 the parts of log p are 1e3 times their sum
            w[key] = max(w[key], loglik_distance(f32["L_S"], f64, "S"), loglik_distance(f32["L_U"], f64, "U"))
            if name in SCORE_CASES:
                w["info"] = max(w["info"], sym_distance(f32["info"], f64["info"]))
    for name in SCORE_CASES:
        p = cases()[name]
        for g, (f64, _) in enumerate(solved(name)):
            # the score is compared at the SAME point: the restatement evaluated at the reference's optimum
            kS, kU, B, logm, r = gene_inputs(p, g)
            at = point32(f64["th"], kS, kU, B, logm, p["W"], p["nuw"], p["noisemodel"], r)
            w["score"] = max(w["score"], score_distance(at["score"], f64))
    for ref, f32 in evaluated().values():
        w["ev_loglik"] = max(w["ev_loglik"], loglik_distance(f32["L_S"], ref, "S"), loglik_distance(f32["L_U"], ref, "U"))
        w["ev_dec"] = max(w["ev_dec"], dec_distance(f32["dec"], ref))
    for name in OUTER_CASES:
        m64, m32, _ = outer_solved(name)
        d = m32["nuw"] - m64["nuw"]
        w["nuw"] = max(w["nuw"], float(math.sqrt(d @ m64["J"] @ d)))
        w["std"] = max(w["std"], float(np.abs(m32["std"] / m64["std"] - 1).max()))
    out = {key: SAFETY * v for key, v in w.items()}
    out["steps"] = steps
    return out
