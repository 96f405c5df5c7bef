"""Checker of the per-gene dispersion estimate (velocycle_amd.gene_harmonics.gene_dispersion / gene_harmonics(dispersion="mle") /
vc_gene_dispersion), written from the formulas.  With eta_c = nu . B[:, c] + a log n_c, mu = exp(eta), r = e^rho = 1 / dispersion:

    L(rho) = sum_c lgamma(k + r) - lgamma(r) + k (eta - ln(r + mu)) - r (ln(r + mu) - ln r)        (+ sum_c -lgamma(k + 1): the log-likelihood)
    f(rho) = L(rho) - (alpha - 1) rho - beta e^-rho                                                (prior shape_inv ~ Gamma(alpha, beta), optional)
    s = dL/dr   = sum_c psi(k + r) - psi(r) - log1p(mu / r) + (mu - k) / (r + mu)
    h = d2L/dr2 = sum_c psi'(k + r) - psi'(r) + 1 / r - 1 / (r + mu) - (mu - k) / (r + mu)^2
    f' = r s - (alpha - 1) + beta / r,     f'' = r^2 h + r s - beta / r

`point_scipy` is these lines with scipy.special's gammaln / digamma / polygamma.  Its differences psi(k + r) - psi(r) carry an absolute
error of eps64 ln r per element, which near the Poisson limit (r = 1e6: the sum s is 4e-8 of its parts) is a tenth of s itself; so the
reference `point64` forms the gamma terms as the sums over j < k of ln(r + j), 1 / (r + j), -1 / (r + j)^2 (counts are integers), element
by element from cumulative sums in extended precision, and tests/test_gene_dispersion_cpu.py holds it to `point_scipy` where that one is
good and to finite differences.  `fit64` is the bracketed Newton iteration on it run to f'^2 / -f'' <= 1e-24, `joint64` the alternation
with gene_glm_checker.newton64 run to |delta rho| <= 1e-12.

`restate` is a restatement of the device kernel's contract: mu by the kernel's recipe (eta float64 from the float32 tables, mu = 2^n 2^f
with one float32 exp2), everything else float64, the gamma terms per element from float64 cumulative sums (not the histogram), sums over
reversed cells, the same bounds, start, noise rule, stopping rules and float32 hand-over of r.  `joint_restate` alternates it with
gene_glm_checker.restate32 under the settling rules of gene_harmonics(dispersion="mle").  The restatement's own distance from the
reference sets the bars (SAFETY x its worst over the GPU cases, as gene_glm_checker does), never the code under test.

Problems come from the regression's own model, mu = exp(nu . zeta(phi)) n^a with Gamma-Poisson counts at a known r per gene
(velocycle_amd.simulate's shape_inv is not the truth of this model)."""
import math
from functools import lru_cache

import numpy as np
from scipy.special import digamma, gammaln, polygamma

from tests.gene_glm_checker import CONVERGED as GLM_CONVERGED
from tests.gene_glm_checker import EPS32, SAFETY, _sum_other_order, basis64, eval64, large_counts, newton64, restate32, solved as glm_solved

EPS64 = float(np.finfo(np.float64).eps)
LOG2E = 1.4426950408889634
RHO_MIN, RHO_MAX = math.log(1e-3), math.log(1e6)
CONVERGED, ROUNDING, AT_UPPER, AT_LOWER, MAX_ITER, EVALUATED, NO_DATA = range(7)
INTERIOR = (CONVERGED, ROUNDING)
T = 1024                       # the kernel's histogram length (csrc/vc_gene_dispersion.hip)
TOL = 1e-10                    # the product's default tol
RHO_TOL, MAX_ROUNDS, START_DISPERSION = 1e-6, 10, 0.3
SEED = 3
LD = np.longdouble


def _prior(prior):
    """(alpha - 1, beta) of a prior that counts, else (0, 0)."""
    if prior is None:
        return 0.0, 0.0
    al, be = float(prior[0]), float(prior[1])
    ok = np.isfinite(al) and np.isfinite(be) and al > 0 and be > 0
    return (al - 1.0, be) if ok else (0.0, 0.0)


def gamma_sums(r, k, dtype=LD):
    """Per element the sums over j < k of ln(r + j), 1 / (r + j), -1 / (r + j)^2 (= lgamma(k + r) - lgamma(r), psi(k + r) - psi(r),
    psi'(k + r) - psi'(r) for integer k): cumulative sums over j in `dtype`, read at k."""
    ki = np.asarray(k).astype(np.int64)
    x = dtype(r) + np.arange(max(int(ki.max(initial=0)), 1), dtype=dtype)
    z = np.zeros(1, dtype)
    tabs = [np.concatenate([z, np.cumsum(t)]) for t in (np.log(x), 1 / x, -1 / (x * x))]
    return [t[ki] for t in tabs]


def histogram_sums(r, k, T_=T):
    """The same three, summed over the gene, by the kernel's route: N_{>j} = #{k > j} for j < T against g(r + j), and for k >= T the
    remainder lgamma(k + r) - lgamma(r + T) and its siblings (scipy here)."""
    k = np.asarray(k, dtype=np.float64)
    j = np.arange(T_, dtype=np.float64)
    ngt = (k[None, :] > j[:, None]).sum(1).astype(np.float64)
    x = r + j
    out = np.array([(ngt * np.log(x)).sum(), (ngt / x).sum(), (-ngt / x ** 2).sum()])
    big = k[k >= T_]
    if big.size:
        out += [t.sum() for t in stirling_differences(r + T_, big - T_)]
    return out


def stirling_differences(x0, dk):
    """lgamma, psi, psi' at x0 + dk minus the same at x0 from Stirling's series, the leading differences written without cancellation
    (the kernel's statements for a count >= T; x0 = r + T >= T: the next terms of the three series are below 1e-24)."""
    x1 = x0 + dk
    i0, i1 = 1 / x0, 1 / x1
    lp = np.log1p(dk * i0)
    cross = dk * (x0 + x1) * i0 ** 2 * i1 ** 2                                  # 1 / x0^2 - 1 / x1^2
    dlg = dk * np.log(x0) + (x1 - 0.5) * lp - dk + (i1 - i0) / 12 - (i1 ** 3 - i0 ** 3) / 360 + (i1 ** 5 - i0 ** 5) / 1260
    dps = lp + 0.5 * dk * i0 * i1 + cross / 12 + (i1 ** 4 - i0 ** 4) / 120 - (i1 ** 6 - i0 ** 6) / 252
    dtg = -dk * i0 * i1 - 0.5 * cross + (i1 ** 3 - i0 ** 3) / 6 - (i1 ** 5 - i0 ** 5) / 30 + (i1 ** 7 - i0 ** 7) / 42
    return dlg, dps, dtg


def point_scipy(r, k, eta, prior=None):
    """(L, f', f'') at r, float64 with scipy.special: the formulas of the head of this file as they stand."""
    pa, pb = _prior(prior)
    mu = np.exp(eta)
    L = (gammaln(k + r) - gammaln(r) + k * (eta - np.log(r + mu)) - r * (np.log(r + mu) - np.log(r))).sum()
    s = (digamma(k + r) - digamma(r) - np.log1p(mu / r) + (mu - k) / (r + mu)).sum()
    h = (polygamma(1, k + r) - polygamma(1, r) + 1 / r - 1 / (r + mu) - (mu - k) / (r + mu) ** 2).sum()
    return float(L), float(r * s - pa + pb / r), float(r * r * h + r * s - pb / r)


def point64(r, k, eta, prior=None):
    """The reference at r: dict(L, fp, fpp, noise (the kernel's noise expression, float64), abs = sum_c |log p_c|)."""
    pa, pb = _prior(prior)
    r_, k_, eta_ = LD(r), np.asarray(k, dtype=LD), np.asarray(eta, dtype=LD)
    mu = np.exp(eta_)
    gl, gs, gh = gamma_sums(r, k)
    lse = np.log(r_ + mu)
    terms = gl + k_ * (eta_ - lse) - r_ * (lse - np.log(r_))
    q = (mu - k_) / (r_ + mu)
    w = np.log1p(mu / r_)
    s = (gs - w + q).sum()
    h = (gh + mu / (r_ * (r_ + mu)) - q / (r_ + mu)).sum()
    noise = 4 * EPS32 * float(np.sqrt(((r_ * mu * q / (r_ + mu)) ** 2).sum())) + 64 * EPS64 * float(r_ * (gs + np.abs(w) + np.abs(q)).sum())
    return dict(L=float(terms.sum()), fp=float(r_ * s - pa + pb / r_), fpp=float(r_ * r_ * h + r_ * s - pb / r_), noise=noise,
                abs=float(np.abs(np.asarray(terms, dtype=np.float64) - gammaln(np.asarray(k, dtype=np.float64) + 1)).sum()))


def moment_start(k, mu):
    den = float(((k - mu) ** 2 - mu).sum())
    r0 = float((mu * mu).sum()) / den if den > 0 else math.exp(RHO_MAX)
    return min(max(math.log(r0), RHO_MIN), RHO_MAX)


def _iterate(point, rho0, tol, max_iter, use_noise):
    """The contract's iteration on `point(r, rho) -> dict(L, fp, fpp, noise)`: bounds first, then the bracketed Newton."""
    p = point(math.exp(RHO_MAX), RHO_MAX)
    if p["fp"] > (-p["noise"] if use_noise else 0.0):
        return dict(p, rho=RHO_MAX, info=float("nan"), iterations=0, status=AT_UPPER)
    p = point(math.exp(RHO_MIN), RHO_MIN)
    if p["fp"] < (p["noise"] if use_noise else 0.0):
        return dict(p, rho=RHO_MIN, info=float("nan"), iterations=0, status=AT_LOWER)
    a, b, rho, steps = RHO_MIN, RHO_MAX, rho0, 0
    if not a < rho < b:
        rho = 0.5 * (a + b)
    while True:
        p = point(math.exp(rho), rho)
        if p["fpp"] < 0 and p["fp"] ** 2 / -p["fpp"] <= tol:
            status = CONVERGED
            break
        if use_noise and abs(p["fp"]) <= p["noise"]:
            status = ROUNDING
            break
        if steps >= max_iter:
            status = MAX_ITER
            break
        if p["fp"] > 0:
            a = rho
        else:
            b = rho
        nt = rho - p["fp"] / p["fpp"] if p["fpp"] < 0 else float("nan")
        rho = nt if a < nt < b else 0.5 * (a + b)
        steps += 1
    return dict(p, rho=rho, info=-p["fpp"], iterations=steps, status=status)


def fit64(k, eta, prior=None, start=None):
    """One gene, the reference: dict(rho, info, std, L, fp, fpp, noise, abs, iterations, status)."""
    rho0 = moment_start(k, np.exp(eta)) if start is None else math.log(start)
    out = _iterate(lambda r, rho: point64(r, k, eta, prior), rho0, 1e-24, 200, False)
    out["std"] = 1 / math.sqrt(out["info"]) if out["info"] > 0 else float("nan")
    return out


def mu32(eta):
    """mu by the kernel's recipe: t = eta log2 e clamped to [-140, 120], mu = 2^rint(t) exp2_float32(t - rint(t))."""
    t = np.clip(np.asarray(eta, dtype=np.float64) * LOG2E, -140.0, 120.0)
    tn = np.rint(t)
    return np.ldexp(np.exp2((t - tn).astype(np.float32)), tn.astype(np.int32)).astype(np.float32)


def eta32(nu, B, logm):
    """eta in float64 from the float32 tables."""
    return np.asarray(nu, dtype=np.float64) @ B.astype(np.float32).astype(np.float64) + logm.astype(np.float32).astype(np.float64)


def point32(r, lnr, k, eta, md, prior=None):
    """One pass of the contract at r: mu (md) carries its float32 rounding, eta stands for ln mu in the large parts."""
    pa, pb = _prior(prior)
    gl, gs, gh = gamma_sums(r, k, np.float64)
    rs = 1 / (r + md)
    big = md >= r
    lg = np.log1p(np.where(big, r, md) / np.where(big, md, r))
    e = eta - lnr
    d, wl = np.where(big, -lg, e - lg), np.where(big, e + lg, lg)
    q = (md - k) * rs
    L = _sum_other_order(gl + k * d - r * wl)
    s = _sum_other_order(gs + q - wl)
    h = _sum_other_order(gh + md * rs / r - q * rs)
    noise = 4 * EPS32 * math.sqrt(_sum_other_order((r * md * q * rs) ** 2)) + 64 * EPS64 * r * _sum_other_order(gs + np.abs(wl) + np.abs(q))
    return dict(L=float(L), fp=float(r * s - pa + pb / r), fpp=float(r * r * h + r * s - pb / r), noise=float(noise))


def restate(k, B, logm, nu, r_start=None, prior=None, tol=TOL, max_iter=50):
    """One gene, the kernel's contract.  r_start: the float32 r the iteration starts from (max_iter == 0: the r evaluated at).
    Returns dict(rho, r32, info, std, L, fp, noise, iterations, status)."""
    k = np.asarray(k, dtype=np.float64)
    eta = eta32(nu, B, logm)
    md = mu32(eta).astype(np.float64)
    if max_iter == 0:
        r = float(np.float32(r_start))
        p = point32(r, math.log(r), k, eta, md, prior)
        out = dict(p, rho=math.log(r), info=-p["fpp"], iterations=0, status=EVALUATED, r32=np.float32(r_start))
    else:
        rho0 = moment_start(k, md) if r_start is None else min(max(math.log(float(np.float32(r_start))), RHO_MIN), RHO_MAX)
        out = _iterate(lambda r, rho: point32(r, rho, k, eta, md, prior), rho0, tol, max_iter, True)
        out["r32"] = np.float32(math.exp(out["rho"]))
    out["std"] = 1 / math.sqrt(out["info"]) if out["info"] > 0 else float("nan")
    return out


def joint64(k, B, logm, prior=None, start_dispersion=START_DISPERSION, max_rounds=100):
    """The reference's alternation: newton64 at r, fit64 at its nu, to |delta rho| <= 1e-12 (or the same bound twice).
    Returns dict(nu, glm (the last newton64), disp (the last fit64), rho, rounds)."""
    rho, last = math.log(1 / start_dispersion), None
    for rnd in range(1, max_rounds + 1):
        glm = newton64(k, B, logm, "NegativeBinomial", math.exp(rho))
        disp = fit64(k, glm["nu"] @ B + logm, prior, start=math.exp(rho))
        done = abs(disp["rho"] - rho) <= 1e-12 or (disp["status"] in (AT_UPPER, AT_LOWER) and disp["status"] == last)
        rho, last = disp["rho"], disp["status"]
        if done:
            break
    glm = newton64(k, B, logm, "NegativeBinomial", math.exp(rho))
    return dict(nu=glm["nu"], glm=glm, disp=disp, rho=rho, rounds=rnd)


def joint_restate(k, B, logm, prior=None, start_dispersion=START_DISPERSION, tol=TOL, rho_tol=RHO_TOL, max_rounds=MAX_ROUNDS):
    """The alternation of gene_harmonics(dispersion="mle") on the two restatements, with the float32 hand-over of r.
    Returns dict(nu, r32, rho, info, std, status, rounds, glm)."""
    r32, rho, last = np.float32(1.0 / start_dispersion), float("nan"), -1
    for rnd in range(1, max_rounds + 1):
        glm = restate32(k, B, logm, "NegativeBinomial", float(r32), tol=tol)
        disp = restate(k, B, logm, glm["nu"], r32, prior, tol)
        settled = disp["r32"] == r32 or abs(disp["rho"] - rho) <= rho_tol or (disp["status"] in (AT_UPPER, AT_LOWER) and disp["status"] == last)
        r32, rho, last = disp["r32"], disp["rho"], disp["status"]
        if settled:
            break
    glm = restate32(k, B, logm, "NegativeBinomial", float(r32), tol=tol)
    return dict(nu=glm["nu"], r32=r32, rho=rho, info=disp["info"], std=disp["std"], status=disp["status"], rounds=rnd, glm=glm)


def stationarity(nu, r, k, B, logm, prior=None):
    """At (nu, r), float64: (|f'| / sqrt(-f'') of the dispersion, the Newton decrement g' H^-1 g of nu)."""
    p = point64(r, k, nu @ B + logm, prior)
    e = eval64(nu, k, B, logm, "NegativeBinomial", r)
    return abs(p["fp"]) / math.sqrt(-p["fpp"]) if p["fpp"] < 0 else float("inf"), float(e["grad"] @ np.linalg.solve(e["hess"], e["grad"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# The problems of tests/test_hip_gene_dispersion.py, built once and shared with tests/test_gene_dispersion_cpu.py.

SHAPES = [(1, 1, 0), (63, 1, 1), (64, 3, 0), (65, 7, 3), (257, 5, 1), (1000, 6, 2), (300, 130, 1)]
EVALUATE_AT = [1e-3, 0.05, 2.0, 1e3, 1e6]
EVALUATE_CASE = "shape_257_5_1"
JOINT_SHAPE = (3000, 40, 1)
POISSON_GENE = 39              # of the joint problem: simulated without overdispersion


def simulate(Nc, Ng, H, seed=SEED, r_lo=0.3, r_hi=5.0, r_true=None, poisson_genes=()):
    """The regression's own model: phases uniform, n_scounts lognormal about 2000, mu = exp(nu . zeta(phi)) n, counts Gamma-Poisson at
    r_true per gene (Poisson for `poisson_genes`, r_true = inf).  Every gene has a count."""
    rng = np.random.default_rng([seed, Nc, Ng, H])
    K = 2 * H + 1
    phis = rng.uniform(0, 2 * np.pi, Nc)
    n = np.maximum(np.rint(rng.lognormal(np.log(2000.0), 0.4, Nc)), 1.0)
    nu = np.zeros((Ng, K))
    nu[:, 0] = np.log(rng.uniform(2.0, 20.0, Ng) / 2000.0)
    for i in range(1, K):
        nu[:, i] = rng.normal(0.0, 0.4 / ((i + 1) // 2), Ng)
    r = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), Ng)) if r_true is None else np.full(Ng, float(r_true))
    B = basis64(phis, H)
    mu = np.exp(nu @ B + np.log(n))
    lam = rng.gamma(r[:, None], mu / r[:, None])
    for g in poisson_genes:
        lam[g], r[g] = mu[g], np.inf
    S = rng.poisson(lam).astype(np.float64).T
    S[0, S.sum(0) == 0] = 1.0
    return dict(S=S, phis=phis, n=n, H=H, nu_true=nu, r_true=r, prior=None)


def _with_nu(p, r_for_fit):
    """Adds nu [Ng, K]: the float64 harmonic fit at r_for_fit per gene (the simulation's nu where that fit does not converge)."""
    B, logm = basis64(p["phis"], p["H"]), np.log(p["n"])
    nu = p["nu_true"].copy()
    for g in range(p["S"].shape[1]):
        fit = newton64(p["S"][:, g], B, logm, "NegativeBinomial", r_for_fit[g])
        if fit["status"] == GLM_CONVERGED:
            nu[g] = fit["nu"]
    return dict(p, nu=nu)


@lru_cache(maxsize=None)
def cases():
    """name -> problem (S [Nc, Ng], phis, n, H, nu [Ng, K], prior (alpha, beta) or None): every problem `gene_dispersion` is held on."""
    out = {}
    for (Nc, Ng, H) in SHAPES:
        p = simulate(Nc, Ng, H)
        out[f"shape_{Nc}_{Ng}_{H}"] = _with_nu(p, p["r_true"])
    for name, extra in (("large_u16", None), ("large_f32", 70000.0)):
        S, phis, n = large_counts(extra)
        nu = glm_solved(f"{name}_NegativeBinomial")[0][0]["nu"]
        out[name] = dict(S=S[:, :1], phis=phis, n=n, H=1, nu=nu[None, :], prior=None)
    rng = np.random.default_rng(SEED)
    one = np.ones(257)
    binary = (rng.uniform(size=257) < 0.3).astype(np.float64)
    out["bound_binary"] = dict(S=binary[:, None], phis=np.zeros(257), n=one, H=0, nu=np.array([[np.log(binary.mean())]]), prior=None)
    binom = rng.binomial(10, 0.5, 257).astype(np.float64)
    out["bound_binomial"] = dict(S=binom[:, None], phis=np.zeros(257), n=one, H=0, nu=np.array([[np.log(5.0)]]), prior=None)
    out["bound_binomial_prior"] = dict(out["bound_binomial"], prior=(2.0, 1.0))
    p = simulate(2000, 1, 0, r_true=5e-4)
    out["bound_lower"] = dict(p, nu=p["nu_true"])
    return out


BOUND_CASES = {"bound_binary": AT_UPPER, "bound_binomial": AT_UPPER, "bound_lower": AT_LOWER}


def gene_inputs(p, g):
    return np.trunc(p["S"][:, g]), basis64(p["phis"], p["H"]), np.log(p["n"])


@lru_cache(maxsize=None)
def solved(name):
    """Per gene of a case: (reference fit, restatement), both at the case's nu."""
    p = cases()[name]
    out = []
    for g in range(p["S"].shape[1]):
        k, B, logm = gene_inputs(p, g)
        out.append((fit64(k, p["nu"][g] @ B + logm, p["prior"]), restate(k, B, logm, p["nu"][g], None, p["prior"])))
    return out


@lru_cache(maxsize=None)
def evaluated():
    """(r32, gene) -> (reference point at float(r32) on the float64 tables, the restatement's evaluate-only pass) of EVALUATE_CASE."""
    p = cases()[EVALUATE_CASE]
    out = {}
    for r in EVALUATE_AT:
        r32 = np.float32(1.0 / (1.0 / r))                                      # the wrapper is handed the dispersion 1 / r
        for g in range(p["S"].shape[1]):
            k, B, logm = gene_inputs(p, g)
            out[(r, g)] = (point64(float(r32), k, p["nu"][g] @ B + logm), restate(k, B, logm, p["nu"][g], r32, None, max_iter=0))
    return out


@lru_cache(maxsize=None)
def joint_problem():
    return simulate(*JOINT_SHAPE, poisson_genes=(POISSON_GENE,))


@lru_cache(maxsize=None)
def joint_solved():
    """Per gene of the joint problem: (joint64, joint_restate)."""
    p = joint_problem()
    B, logm = basis64(p["phis"], p["H"]), np.log(p["n"])
    return [(joint64(p["S"][:, g], B, logm), joint_restate(p["S"][:, g], B, logm)) for g in range(p["S"].shape[1])]


def fit_distances(got_rho, got_std, ref):
    """rho in standard errors of the reference, log_r_std relative."""
    return dict(rho=abs(got_rho - ref["rho"]) * math.sqrt(ref["info"]), std=abs(got_std / ref["std"] - 1))


def point_distances(got_loglik, got_score, ref):
    """loglik (without -lgamma(k + 1), as the kernel returns it) in eps32 sum_c |log p_c|, the score in the noise rule's units."""
    return dict(loglik=abs(got_loglik - ref["L"]) / (EPS32 * ref["abs"]), score=abs(got_score - ref["fp"]) / ref["noise"])


@lru_cache(maxsize=None)
def worst():
    """The restatement's worst distance from the reference over the GPU cases, per yardstick."""
    w = dict(rho=0.0, std=0.0, loglik=0.0, score=0.0, stat_r=0.0, stat_nu=0.0)
    for name in cases():
        for (f64, f32) in solved(name):
            if f64["status"] == CONVERGED and f32["status"] in INTERIOR:
                for key, v in fit_distances(f32["rho"], f32["std"], f64).items():
                    w[key] = max(w[key], v)
    for (ref, f32) in evaluated().values():
        for key, v in point_distances(f32["L"], f32["fp"], ref).items():
            w[key] = max(w[key], v)
    p = joint_problem()
    B, logm = basis64(p["phis"], p["H"]), np.log(p["n"])
    for g, (_, f32) in enumerate(joint_solved()):
        sr, dn = stationarity(f32["nu"], float(f32["r32"]), p["S"][:, g], B, logm)
        if f32["status"] in INTERIOR:
            w["stat_r"] = max(w["stat_r"], sr)
        w["stat_nu"] = max(w["stat_nu"], dn)
    return w


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst per yardstick; rho gets sqrt(tol) more: two correct iterations that both stop at
    f'^2 / -f'' <= tol may differ by that many standard errors."""
    b = {key: SAFETY * v for key, v in worst().items()}
    b["rho"] += math.sqrt(TOL)
    return b


def overdispersion_p(lr):
    """0.5 * the chi-square(1) survival function: the boundary mixture's p-value at lr > 0."""
    return 0.5 * math.erfc(math.sqrt(max(float(lr), 0.0) / 2))
