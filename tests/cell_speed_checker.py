"""Checker of the per-cell and per-group angular speed (velocycle_amd.cell_speed / vc_cell_speed), written from the formulas.  The model is
gene_kinetics_checker's with the roles swapped: x = log gamma, y = log beta of every gene are given, and the angular speed om of a cell
(or of a group of cells) is the unknown.  Per cell c and gene g, B = [1, sin phi, cos phi, ...]:

    etaS = nu_g . B_c + logm_c,   d = nu_g . dB_c,   z = om d + e^x_g,   a = [z > 0],   zp = a z + 1e-5
    etaU = etaS - y_g + ln zp,   mu = e^etaU,   q = a d / zp
    res = k - mu | (k - mu) r / (r + mu),   w (Fisher) = mu | mu r / (r + mu),   wo (observed) = mu | mu r (k + r) / (r + mu)^2
    L = sum log p(k | mu),   score = sum res q,   fisher = sum w q^2,   observed = sum (wo + res) q^2,   N = sum (wo^2 + res^2) q^2
    f = L - (om - m)^2 / 2 s^2,   G = score - (om - m) / s^2,   A = observed + 1 / s^2 where positive, else fisher + 1 / s^2

the sums over the genes of a cell, or over the genes of every cell of a group.  `point64` is these lines in float64 from float64
tables; `solve64` the Newton iteration (step G / A, halved while f drops) run to dec <= 1e-24 max(1, |f|).

`point32` restates the device kernel's contract: tables rounded to float32, etaS, d, z and etaS - y float64, e^(etaS - y) rounded once
to float32 and multiplied by zp in float32, the residual, the weights, the NB logarithm and ln zp float32, float64 sums over reversed
elements; `solve32` runs the contract's rules on it (tol, the rounding rule, the halving allowance 8 eps32 max(A, A'), the box
[-30, 30]).  The restatement's own distance from the reference sets every bar (SAFETY x its worst over the GPU cases, as
gene_kinetics_checker does), never the code under test.

Problems come from gene_kinetics_checker.simulate with its x, y as the kinetics; seeds are fixed.  Tolerance-bearing cases are kink-free
(min z >= MIN_Z at every point the reference visits) and at least 90 % of their cells are CONVERGED in the reference: `bars` asserts
both for every case."""
import math
from functools import lru_cache

import numpy as np
from scipy.special import gammaln

from tests.gene_glm_checker import EPS32, SAFETY, _sum_other_order, basis64, logp64
from tests.gene_kinetics_checker import (BOUND, CONVERGED, EPS64, EVALUATED, FLOOR, HALVINGS, INTERIOR, MAX_ITER, MIN_Z, NB, NO_DATA, PO,
                                         ROUNDING, UNBOUNDED, simulate)

TOL, MAX_ITER_DEFAULT, START = 1e-10, 25, 0.4
GROUP_PRIOR = (0.0, 3.0)                   # AngularSpeed.trivial_prior's constant
MIN_CONVERGED = 0.9

# (Nc, Ng, H, noise, extra arguments of simulate): seeds 100 + i.  One cell, the wave's and the workgroup's edges, gene counts that do
# and do not divide by the four waves
SHAPES = [(65, 64, 1, PO, {}),
          (257, 3, 1, PO, dict(level=(4.5, 5.5), gamma_range=(0.0, 0.5))),
          (1, 257, 2, NB, {}),
          (130, 1, 1, PO, dict(level=(5.5, 6.0), gamma_range=(0.2, 0.5))),
          (64, 65, 2, NB, dict(level=(4.5, 5.5), gamma_range=(0.2, 0.5))),       # the defaults reach min z 0.025
          (63, 4, 2, PO, dict(level=(4.5, 5.5), gamma_range=(0.0, 0.5))),
          (64, 5, 1, PO, dict(level=(5.5, 6.0), gamma_range=(0.2, 0.5)))]
KINK_CASE = "kink_63_5"                    # 63 x 5, NB, defaults: kinks, omega to +-3: not a tolerance case
LARGE_CASES = ["large_u16", "large_f32"]
GROUP_CASES = ["bins_1025_12", "conditions_1025_12"]
EVALUATE_CASE = "shape_65_64_1_Poisson"
EVALUATE_AT = [0.4, 0.0, 0.9, -0.3, -2.5]  # the last one clamps genes


def shape_name(Nc, Ng, H, noise):
    return f"shape_{Nc}_{Ng}_{H}_{noise}"


FIT_CASES = [shape_name(*s[:4]) for s in SHAPES] + LARGE_CASES


@lru_cache(maxsize=None)
def cases():
    out = {}
    for i, (Nc, Ng, H, noise, extra) in enumerate(SHAPES):
        out[shape_name(Nc, Ng, H, noise)] = simulate(100 + i, Nc, Ng, H, noise, [0.4], **extra)
    out[KINK_CASE] = simulate(105, 63, 5, 1, NB, [0.4])
    out["large_u16"] = simulate(110, 65, 5, 1, PO, [0.4], level=(4.0, 4.5), gamma_range=(0.0, 0.5), big=800.0)
    out["large_f32"] = simulate(111, 65, 64, 1, NB, [0.4], level=(4.0, 4.5), gamma_range=(0.2, 0.5), big=2600.0)
    out["bins_1025_12"] = simulate(120, 1025, 12, 1, NB, [0.4, 0.1, -0.1], Hw=1)
    out["conditions_1025_12"] = simulate(121, 1025, 12, 1, PO, [0.45, 0.3], Nx=2, level=(4.0, 5.5))
    return out


def true_speed(p):
    return p["nuw"] @ p["W"]


def phase_bins(p, bins):
    """groups [Nc] = condition x bins + phase bin, and their number."""
    j = np.minimum((np.mod(p["phis"], 2 * np.pi) / (2 * np.pi) * bins).astype(np.int64), bins - 1)
    x = np.zeros(len(j), dtype=np.int64) if p["D"] is None else p["D"].argmax(0)
    return x * bins + j, bins * p["Nx"]


GROUPS = {"bins_1025_12": 8, "conditions_1025_12": 4}


# ---------------------------------------------------------------------------------------------------------------- tables
@lru_cache(maxsize=None)
def tables(name, f32=False):
    """etaS [Nc, Ng] and d [Nc, Ng] in float64 from the float64 tables, or (f32) from the tables rounded to float32."""
    p = cases()[name]
    B, logm = basis64(p["phis"], p["H"]), np.log(p["n"])
    if f32:
        B, logm = B.astype(np.float32).astype(np.float64), logm.astype(np.float32).astype(np.float64)
    nu = p["nu"]
    etaS = (nu @ B).T + logm[:, None]
    d = np.zeros_like(etaS)
    for h in range(1, p["H"] + 1):
        d = d + h * (B[2 * h][:, None] * nu[None, :, 2 * h - 1] - B[2 * h - 1][:, None] * nu[None, :, 2 * h])
    return etaS, d


def _finish(om, a, z, zp, d, res, w, wo, L, A, prior, other_order, extra):
    S = (lambda v: float(_sum_other_order(np.ravel(v)))) if other_order else (lambda v: float(np.asarray(v, dtype=np.float64).sum()))
    m, pp = (0.0, 0.0) if prior is None else (prior[0], 1.0 / prior[1] ** 2)
    q = np.where(a, d / zp, 0.0)
    q2 = q * q
    score, fisher, observed, N = S(res * q), S(w * q2), S((wo + res) * q2), S((wo * wo + res * res) * q2)
    G = score - pp * (om - m)
    M = observed + pp
    if not (0.0 < M < 1e300):
        M = fisher + pp
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        step = G / M
        dec = G * step
    return dict(om=om, L=L, A=A, f=L - 0.5 * pp * (om - m) ** 2, score=score, fisher=fisher, observed=observed, N=N, G=G, M=M, step=step,
                dec=dec, n_clamped=int((~a).sum()), minz=float(z.min()), se=1.0 / math.sqrt(fisher + pp) if fisher + pp > 0 else np.nan,
                **extra)


def point64(om, k, etaS, d, x, y, noisemodel, r=None, prior=None):
    """The reference at om over the elements handed in (any shape [..., Ng]).  L is the FULL log-likelihood; abs = sum |log p|."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        z = om * d + np.exp(x)
        a = z > 0
        zp = np.where(a, z, 0.0) + FLOOR
        etaU = etaS - y + np.log(zp)
        mu = np.exp(etaU)
        if noisemodel == "Poisson":
            res, w, wo = k - mu, mu, mu
        else:
            res, w, wo = (k - mu) * r / (r + mu), mu * r / (r + mu), mu * r * (k + r) / (r + mu) ** 2
        lp = logp64(k, etaU, noisemodel, r)
        parts = np.abs(k * etaU) + gammaln(k + 1) + (mu if noisemodel == "Poisson" else
                                                     gammaln(k + r) + np.abs(gammaln(r)) + np.abs(r * np.log(r)) + (k + r) * np.abs(np.log(r + mu)))
        return _finish(om, a, z, zp, d, res, w, wo, float(lp.sum()), float(parts.sum()), prior, False, dict(abs=float(np.abs(lp).sum())))


def constants64(k, noisemodel, r):
    """The part of the log-likelihood the kernel's objective leaves out (its NB objective holds r ln r)."""
    if noisemodel == "Poisson":
        return float(-gammaln(k + 1).sum())
    return float((gammaln(k + r) - gammaln(r) - gammaln(k + 1)).sum())


def point32(om, k, etaS, d, x, y, noisemodel, r=None, prior=None):
    """The kernel's contract at om: etaS, d from the float32 tables (`tables(name, True)`).  L is the full log-likelihood (the float64
    constants added), A the kernel's sum |terms|."""
    f32 = np.float32
    k32 = k.astype(f32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        z = om * d + np.exp(x)
        a = z > 0
        zp = np.where(a, z + FLOOR, FLOOR)
        e0 = etaS - y
        zpf = zp.astype(f32)
        mu = np.exp(e0).astype(f32) * zpf
        etaU = e0 + np.log(zpf).astype(np.float64)
        kd = k32.astype(np.float64)
        if noisemodel == "Poisson":
            res, w, wo = k32 - mu, mu, mu
            terms = kd * etaU - mu.astype(np.float64)
            mag = np.abs(kd * etaU) + mu.astype(np.float64)
            r64 = None
        else:
            r32 = np.broadcast_to(np.asarray(r), k.shape[-1:]).astype(f32)
            s = r32 + mu
            pr = r32 / s
            res, w, wo = (k32 - mu) * pr, mu * pr, (mu / s) * pr * (k32 + r32)
            big = mu >= r32
            xx = np.where(big, r32, mu) / np.where(big, mu, r32)
            lg = np.log(f32(1) + xx.astype(f32)).astype(np.float64)
            r64 = r32.astype(np.float64)
            lnr = np.log(r64)
            e = etaU - lnr
            terms = kd * np.where(big, -lg, e - lg) - r64 * np.where(big, e + lg, lg)
            mag = (kd + r64) * np.abs(np.where(big, etaU, lnr) + lg) + np.abs(kd * etaU)
        L = float(_sum_other_order(np.ravel(terms))) + constants64(k, noisemodel, r64)
        return _finish(om, a, z, zp, d, res.astype(np.float64), w.astype(np.float64), wo.astype(np.float64), L,
                       float(_sum_other_order(np.ravel(mag))), prior, True, {})


# ---------------------------------------------------------------------------------------------------------------- iteration
def _iterate(point, om, tol, max_iter, eps, rounding_rule):
    """The contract's iteration on `point(om)`.  tol: a number, or a function of the point (the reference's relative tolerance).
    minz_path: the least z over every point visited, refused trials included."""
    om = min(max(om, -BOUND), BOUND)
    e = point(om)
    minz = e["minz"]
    if max_iter == 0:
        return dict(e, iterations=0, status=EVALUATED, minz_path=minz)
    steps, halvings, status = 0, HALVINGS, MAX_ITER
    while True:
        if not abs(e["dec"]) < 1e300:
            break
        if e["dec"] <= (tol(e) if callable(tol) else tol):
            status = CONVERGED
            break
        if rounding_rule and abs(e["G"]) <= 4 * EPS32 * math.sqrt(e["N"]):
            status = ROUNDING
            break
        if steps >= max_iter:
            break
        t, moved = 1.0, False
        while True:
            tr = e["om"] + t * e["step"]
            if not abs(tr) <= BOUND:
                status = UNBOUNDED
                break
            trial = point(tr)
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
    return dict(e, iterations=steps, status=status, minz_path=minz)


def _no_data():
    nan = float("nan")
    return dict(om=nan, L=nan, A=nan, f=nan, score=nan, fisher=nan, observed=nan, N=nan, G=nan, M=nan, step=nan, dec=nan, n_clamped=0,
                minz=nan, se=nan, abs=nan, iterations=0, status=NO_DATA, minz_path=nan)


def _elements(name, rows, f32):
    p = cases()[name]
    etaS, d = tables(name, f32)
    return p["U"][rows], etaS[rows], d[rows], p["x"], p["y"], p["noisemodel"], p["r"]


def solve64(name, rows, start=START, prior=None, max_iter=60):
    """The reference over the cells `rows` of a case (one cell: [c]; a group: its cells) sharing one om."""
    el = _elements(name, rows, False)
    if not el[0].sum() > 0:
        return _no_data()
    return _iterate(lambda om: point64(om, *el, prior), start, lambda e: 1e-24 * max(1.0, abs(e["f"])), max_iter, EPS64, False)


def solve32(name, rows, start=START, prior=None, tol=TOL, max_iter=MAX_ITER_DEFAULT):
    el = _elements(name, rows, True)
    if not el[0].sum() > 0:
        return _no_data()
    return _iterate(lambda om: point32(om, *el, prior), start, tol, max_iter, EPS32, True)


def at64(name, rows, om, prior=None):
    return point64(om, *_elements(name, rows, False), prior)


def at32(name, rows, om, prior=None):
    return point32(om, *_elements(name, rows, True), prior)


@lru_cache(maxsize=None)
def solved(name, prior=None):
    """Per cell (reference, restatement) of a case from START."""
    Nc = cases()[name]["U"].shape[0]
    return [(solve64(name, [c], prior=prior), solve32(name, [c], prior=prior)) for c in range(Nc)]


@lru_cache(maxsize=None)
def group_solved(name):
    """Per group (reference, restatement, the cells) of a grouped case from START under GROUP_PRIOR."""
    p = cases()[name]
    grp, G = phase_bins(p, GROUPS[name])
    out = []
    for g in range(G):
        rows = np.flatnonzero(grp == g)
        out.append((solve64(name, rows, prior=GROUP_PRIOR), solve32(name, rows, prior=GROUP_PRIOR), rows))
    return out


@lru_cache(maxsize=None)
def evaluated():
    """{(i, c): (reference, restatement)} at EVALUATE_AT[i] of EVALUATE_CASE."""
    Nc = cases()[EVALUATE_CASE]["U"].shape[0]
    return {(i, c): (at64(EVALUATE_CASE, [c], om), at32(EVALUATE_CASE, [c], om)) for i, om in enumerate(EVALUATE_AT) for c in range(Nc)}


# ---------------------------------------------------------------------------------------------------------------- distances and bars
def omega_distance(om, ref):
    """|delta| in standard errors of the reference: |delta| sqrt(A64)."""
    return abs(om - ref["om"]) * math.sqrt(ref["M"])


def rel_distance(got, ref):
    return abs(got / ref - 1.0)


def loglik_distance(L, ref):
    return abs(L - ref["L"]) / (EPS32 * ref["abs"])


def score_distance(score, ref):
    return abs(score - ref["score"]) / (4 * EPS32 * math.sqrt(ref["N"]))


def check_case(name):
    """What a tolerance-bearing per-cell case must hold in the reference: kink-free along every path, >= 90 % of the cells CONVERGED.
    Returns the list of (cell, reference, restatement) of the cells CONVERGED in the reference and interior in the restatement."""
    sol = solved(name)
    live = [(c, f64, f32) for c, (f64, f32) in enumerate(sol) if f64["status"] != NO_DATA]
    minz = min(f64["minz_path"] for _, f64, _ in live)
    assert minz >= MIN_Z, (name, minz)
    conv = [(c, f64, f32) for c, f64, f32 in live if f64["status"] == CONVERGED]
    assert len(conv) >= MIN_CONVERGED * len(sol), (name, len(conv), len(sol))
    assert all(f32["status"] in INTERIOR for _, _, f32 in conv), name
    return conv


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst distance from the reference over the GPU cases, per asserted figure."""
    w = dict(omega=0.0, var=0.0, fisher=0.0, observed=0.0, loglik=0.0, loglik_large=0.0, score=0.0, ev_loglik=0.0, ev_score=0.0, group=0.0,
             group_std=0.0)
    for name in FIT_CASES:
        for c, f64, f32 in check_case(name):
            w["omega"] = max(w["omega"], omega_distance(f32["om"], f64))
            w["var"] = max(w["var"], rel_distance(1.0 / f32["M"], 1.0 / f64["M"]))
            w["fisher"] = max(w["fisher"], rel_distance(f32["fisher"], f64["fisher"]))
            w["observed"] = max(w["observed"], rel_distance(f32["observed"], f64["observed"]))
            key = "loglik_large" if name in LARGE_CASES else "loglik"      # at counts of 1e4 the parts of log p are 1e3 times their sum
            w[key] = max(w[key], loglik_distance(f32["L"], f64))
            # the score is compared at the SAME point: the restatement evaluated at the reference's optimum
            w["score"] = max(w["score"], score_distance(at32(name, [c], f64["om"])["score"], f64))
    for ref, f32 in evaluated().values():
        w["ev_loglik"] = max(w["ev_loglik"], loglik_distance(f32["L"], ref))
        w["ev_score"] = max(w["ev_score"], score_distance(f32["score"], ref))
    for name in GROUP_CASES:
        for f64, f32, rows in group_solved(name):
            assert f64["status"] == CONVERGED and f32["status"] in INTERIOR and f64["minz_path"] >= MIN_Z, (name, f64["status"], f64["minz_path"])
            w["group"] = max(w["group"], omega_distance(f32["om"], f64))
            w["group_std"] = max(w["group_std"], rel_distance(f32["se"], f64["se"]))
    return {key: SAFETY * v for key, v in w.items()}
