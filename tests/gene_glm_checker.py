"""Checker of the per-gene harmonic regression (Cycle.from_phases_mle / velocycle_amd.gene_harmonics / vc_gene_glm), written from the
formulas:

    eta_c = nu . B[:, c] + a log n_c,   B = [1, sin phi, cos phi, sin 2 phi, ...],   mu = exp(eta)
    Poisson            log p = k eta - mu - lgamma(k + 1)
    NegativeBinomial   log p = lgamma(k + r) - lgamma(r) - lgamma(k + 1) + r log r + k eta - (k + r) log(r + mu),   r = 1 / dispersion
    objective          sum_c log p  -  sum_i (nu_i - m_i)^2 / (2 s_i^2)             (the Gaussian prior is optional)
    gradient           sum_c res B_i,   res = k - mu | (k - mu) r / (r + mu)
    observed Hessian   sum_c w B_i B_j, w = mu | mu r (k + r) / (r + mu)^2,         1 / s_i^2 on the diagonal
    start              nu_0 = log(sum k / sum n^a), harmonics 0 (prior means, except nu_0)

`newton64` is the float64 reference: undamped Newton to dec = g' H^-1 g <= 1e-24 max(1, |L|) or 60 iterations.  `restate32` is a
float32 restatement of the device kernel's contract -- float32 tables, eta formed in float64 from them, then mu, the residual, the weight,
the logarithm and the terms k eta, (k + r) log(r + mu) of the log-probability each a float32 number, float64 sums in another order (numpy's
pairwise sums over reversed cells), the same step and stopping rules -- whose own distance from float64 sets the bars (SAFETY x its
worst, as tests/mle_checker.py does).  (With eta itself rounded to float32 the gradient's noise at counts of 10^4 is as large as the
ROUNDING rule's threshold, and the constant-only fit of such a gene wanders until max_iter: the contract asks for float64 there.)

Yardsticks (scale-free): coefficients  sqrt(d' H64 d)  (standard errors);  stds  |std / std64 - 1|;  loglik and lr_stat
|x - x64| / (eps32 sum_c |log p_c|) at the float64 optimum."""
import math
from functools import lru_cache

import numpy as np
from scipy.special import gammaln

EPS32 = float(np.finfo(np.float32).eps)
SAFETY = 4.0
COEF_CAP = 1e-3                # the coefficient bar may not exceed this many standard errors
CONVERGED, ROUNDING, UNBOUNDED, SINGULAR, MAX_ITER = 0, 1, 2, 3, 4
BOUND = 50.0
HALVINGS = 30
SEED = 1


def basis64(phis, H):
    """[2H+1, Nc] float64 from the angles themselves (the product forms it from the directions by angle addition)."""
    phis = np.asarray(phis, dtype=np.float64)
    rows = [np.ones_like(phis)]
    for k in range(1, H + 1):
        rows += [np.sin(k * phis), np.cos(k * phis)]
    return np.stack(rows)


def logp64(k, eta, noisemodel, r):
    """Full log-probability per element, float64."""
    mu = np.exp(eta)
    if noisemodel == "Poisson":
        return k * eta - mu - gammaln(k + 1)
    return gammaln(k + r) - gammaln(r) - gammaln(k + 1) + r * np.log(r) + k * eta - (k + r) * np.log(r + mu)


def eval64(nu, k, B, logm, noisemodel, r=None, pm=None, pp=None):
    """At nu [K]: dict(loglik (full, without the prior), objective (with it), grad, hess (with the prior), abs = sum_c |log p_c|)."""
    eta = nu @ B + logm
    mu = np.exp(eta)
    if noisemodel == "Poisson":
        res, w = k - mu, mu
    else:
        res, w = (k - mu) * r / (r + mu), mu * r * (k + r) / (r + mu) ** 2
    lp = logp64(k, eta, noisemodel, r)
    grad = B @ res
    hess = (B * w) @ B.T
    obj = lp.sum()
    if pm is not None:
        d = nu - pm
        grad = grad - pp * d
        hess = hess + np.diag(pp)
        obj = obj - 0.5 * (pp * d * d).sum()
    return dict(loglik=lp.sum(), objective=obj, grad=grad, hess=hess, abs=np.abs(lp).sum())


def _prior(prior, K):
    if prior is None:
        return None, None
    pm, ps = np.asarray(prior[0], dtype=np.float64), np.asarray(prior[1], dtype=np.float64)
    has = np.isfinite(pm) & np.isfinite(ps)
    return np.where(has, pm, 0.0), np.where(has, 1.0 / np.where(has, ps, 1.0) ** 2, 0.0)


def start(k, logm, K, pm, pp):
    nu = np.zeros(K)
    if pm is not None:
        nu = np.where(pp > 0, pm, 0.0)
    nu[0] = math.log(k.sum() / np.exp(logm).sum())
    return nu


def newton64(k, B, logm, noisemodel, r=None, prior=None, max_iter=60):
    """One gene.  Returns dict(nu, hess, cov, std, loglik, abs, dec, iterations, status)."""
    K = B.shape[0]
    pm, pp = _prior(prior, K)
    nu = start(k, logm, K, pm, pp)
    status = MAX_ITER
    for it in range(max_iter + 1):
        e = eval64(nu, k, B, logm, noisemodel, r, pm, pp)
        try:
            step = np.linalg.solve(e["hess"], e["grad"])
            np.linalg.cholesky(e["hess"])
        except np.linalg.LinAlgError:
            status = SINGULAR
            break
        dec = float(e["grad"] @ step)
        if not np.isfinite(dec):
            status = SINGULAR
            break
        if dec <= 1e-24 * max(1.0, abs(e["objective"])):
            status = CONVERGED
            break
        if it == max_iter:
            break
        nu = nu + step
        if np.abs(nu[1:]).max(initial=0.0) > BOUND:
            status = UNBOUNDED
            break
    cov = np.linalg.inv(e["hess"]) if status == CONVERGED else np.full((K, K), np.nan)
    return dict(nu=nu, hess=e["hess"], cov=cov, std=np.sqrt(np.diag(cov)), loglik=e["loglik"], abs=e["abs"], dec=dec, iterations=it,
                status=status)


def _sum_other_order(x):
    """float64 sum over the last axis, cells reversed (numpy sums pairwise): another order than the kernel's strided lanes."""
    return np.asarray(x, dtype=np.float64)[..., ::-1].sum(-1)


def eval32(nu, k32, B32, logm32, noisemodel, r32, const64):
    """The sums of one pass at nu with float32 per-element terms: grad, hess, loglik (full), A = sum |terms|, N_i (rounding scale)."""
    eta = nu @ B32.astype(np.float64) + logm32.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        mu = np.exp(eta).astype(np.float32)
        t1 = (k32 * eta).astype(np.float32)
        if noisemodel == "Poisson":
            res, w = k32 - mu, mu
            t2 = mu
        else:
            s = r32 + mu
            res, w = (k32 - mu) * (r32 / s), (mu / s) * (r32 / s) * (k32 + r32)
            t2 = (k32 + r32) * np.log(s)
        grad = _sum_other_order(res.astype(np.float64) * B32)
        hess = np.einsum("ic,jc->ij", (B32 * w.astype(np.float64))[:, ::-1], B32.astype(np.float64)[:, ::-1])
        N = _sum_other_order((w.astype(np.float64) ** 2 + res.astype(np.float64) ** 2) * B32.astype(np.float64) ** 2)
        L = _sum_other_order(t1) - _sum_other_order(t2)
        A = _sum_other_order(np.abs(t1)) + _sum_other_order(np.abs(t2))
    return dict(grad=grad, hess=hess, L=L, A=A, N=N, loglik=L + const64)


def constants64(k, noisemodel, r):
    """sum_c of the terms of log p that do not depend on nu."""
    if noisemodel == "Poisson":
        return float(-gammaln(k + 1).sum())
    return float((gammaln(k + r) - gammaln(r) - gammaln(k + 1) + r * np.log(r)).sum())


def restate32(k, B, logm, noisemodel, r=None, prior=None, tol=1e-10, max_iter=25, rounding_rule=True):
    """One gene, the kernel's contract in float32 terms.  Returns dict(nu, cov, std, loglik, dec, iterations, status)."""
    K = B.shape[0]
    pm, pp = _prior(prior, K)
    k32, B32, logm32 = k.astype(np.float32), B.astype(np.float32), logm.astype(np.float32)
    r32 = np.float32(r) if r is not None else None
    const = constants64(k, noisemodel, float(r32) if r32 is not None else None)
    nu = start(k, logm32.astype(np.float64), K, pm, pp)

    def penalised(e, x):
        g, h, pen = e["grad"], e["hess"], 0.0
        if pm is not None:
            d = x - pm
            g, h, pen = g - pp * d, h + np.diag(pp), 0.5 * (pp * d * d).sum()
        return g, h, pen

    e = eval32(nu, k32, B32, logm32, noisemodel, r32, const)
    status, steps, halvings, dec = MAX_ITER, 0, HALVINGS, float("nan")
    cov = np.full((K, K), np.nan)
    while True:
        g, h, pen = penalised(e, nu)
        try:
            np.linalg.cholesky(h)
            dx = np.linalg.solve(h, g)
            cov = np.linalg.inv(h)
        except np.linalg.LinAlgError:
            status, cov = SINGULAR, np.full((K, K), np.nan)
            break
        dec = float(g @ dx)
        if not np.isfinite(dec):
            status = SINGULAR
            break
        if dec <= tol:
            status = CONVERGED
            break
        if rounding_rule and (np.abs(g) <= 4 * EPS32 * np.sqrt(e["N"])).all():
            status = ROUNDING
            break
        if steps >= max_iter:
            break
        t, moved = 1.0, False
        while True:
            trial = nu + t * dx
            if np.abs(trial[1:]).max(initial=0.0) > BOUND:
                status = UNBOUNDED
                break
            e2 = eval32(trial, k32, B32, logm32, noisemodel, r32, const)
            pen2 = penalised(e2, trial)[2]
            if e2["L"] - pen2 >= e["L"] - pen - 8 * EPS32 * max(e["A"], e2["A"]):
                nu, e, moved = trial, e2, True
                break
            if halvings == 0:
                break
            halvings -= 1
            t *= 0.5
        if not moved:
            break
        steps += 1
    return dict(nu=nu, cov=cov, std=np.sqrt(np.diag(cov)), loglik=e["loglik"], dec=dec, iterations=steps, status=status)


def distances(got_nu, got_std, got_ll, got_lr, ref, ref_null):
    """The four yardsticks of one gene against its float64 fits (full model `ref`, constant alone `ref_null`)."""
    d = np.asarray(got_nu, dtype=np.float64) - ref["nu"]
    scale = EPS32 * ref["abs"]
    return dict(coef=float(np.sqrt(max(d @ ref["hess"] @ d, 0.0))), std=float(np.abs(np.asarray(got_std) / ref["std"] - 1).max()),
                loglik=float(abs(got_ll - ref["loglik"]) / scale),
                lr=float(abs(got_lr - 2 * (ref["loglik"] - ref_null["loglik"])) / scale))


# ---------------------------------------------------------------------------------------------------------------------------------
# The problems of tests/test_hip_gene_harmonics.py, built once and shared with tests/test_gene_harmonics_cpu.py (which derives the bars
# from them and asserts that every float64 fit converges).

SHAPES = [(63, 1, 1), (64, 3, 0), (65, 7, 3), (255, 5, 2), (257, 5, 1), (1000, 3, 3), (300, 130, 1)]
NOISES = [("Poisson", None), ("NegativeBinomial", 0.3)]


@lru_cache(maxsize=None)
def simulated(Nc, Ng, seed=SEED):
    """counts [Nc, Ng] float64, phis float64 [Nc], n_scounts = max(row sum, 1), and the simulation's truth."""
    from velocycle_amd.simulate import simulate_counts
    sim = simulate_counts(Nc=Nc, Ng=Ng, seed=seed)
    S = sim["S"].double().numpy()
    return dict(S=S, phis=sim["phis"].double().numpy(), n=np.maximum(S.sum(1), 1.0), nu=sim["nu"].double().numpy(),
                shape_inv=sim["shape_inv"].double().numpy())


def problem(S, phis, n, H, noisemodel, dispersion=None, prior=None, a=1.0):
    """A problem as the tests hand it around.  dispersion: scalar or [Ng]; prior: (means [K, Ng], stds [K, Ng]) or None."""
    return dict(S=np.asarray(S, dtype=np.float64), phis=np.asarray(phis, dtype=np.float64), n=np.asarray(n, dtype=np.float64), H=H,
                noisemodel=noisemodel, dispersion=dispersion, prior=prior, a=a)


def directions(phis):
    return np.stack([np.cos(phis), np.sin(phis)])


def large_counts(extra=None):
    """Gene 0 of the (257, 16) problem times 2000 (counts reach 10^4); n_scounts stay those of the unscaled matrix.  extra: a count
    that replaces the first one of gene 0 (70 000 forces float32 storage)."""
    sim = simulated(257, 16)
    S = sim["S"].copy()
    S[:, 0] *= 2000
    if extra is not None:
        S[0, 0] = extra
    return S, sim["phis"], sim["n"]


def separated():
    """The (257, 5) problem with a sixth gene that has the counts 1, 2, 1 in three cells and none elsewhere."""
    sim = simulated(257, 5)
    col = np.zeros((257, 1))
    col[[10, 100, 200], 0] = [1, 2, 1]
    return np.hstack([sim["S"], col]), sim["phis"], sim["n"]


PERMUTED_GENE = 4              # the most periodic gene of the (3000, 8) problem


def permutation(Nc):
    """The cells' phases dealt out anew: counts and n_scounts stay paired, the phases carry no information about them."""
    return np.random.default_rng(1).permutation(Nc)


def separation_prior(Ng, H=3):
    K = 2 * H + 1
    return np.zeros((K, Ng)), np.vstack([np.full((1, Ng), 10.0), np.ones((K - 1, Ng))])


@lru_cache(maxsize=None)
def cases():
    """name -> problem: every problem the GPU tests hold against the bars."""
    out = {}
    for (Nc, Ng, H) in SHAPES:
        sim = simulated(Nc, Ng)
        for noise, disp in NOISES:
            out[f"shape_{Nc}_{Ng}_{H}_{noise}"] = problem(sim["S"], sim["phis"], sim["n"], H, noise, disp)
    for noise, disp in NOISES:
        out[f"large_u16_{noise}"] = problem(*large_counts(), 1, noise, disp)
        out[f"large_f32_{noise}"] = problem(*large_counts(70000.0), 1, noise, disp)
    S, phis, n = separated()
    out["separation_prior"] = problem(S, phis, n, 3, "Poisson", None, separation_prior(S.shape[1]))
    sim = simulated(257, 5)
    K = 3
    out["prior_wide"] = problem(sim["S"], sim["phis"], sim["n"], 1, "NegativeBinomial", 0.3,
                                (np.zeros((K, 5)), np.full((K, 5), 1e6)))
    sim = simulated(3000, 8)
    out["periodicity"] = problem(sim["S"], sim["phis"], sim["n"], 1, "NegativeBinomial", 0.3)
    out["permuted"] = problem(sim["S"][:, PERMUTED_GENE:PERMUTED_GENE + 1], sim["phis"][permutation(3000)], sim["n"], 1,
                              "NegativeBinomial", 0.3)
    sim = simulated(255, 5)
    out["per_gene_dispersion"] = problem(sim["S"], sim["phis"], sim["n"], 2, "NegativeBinomial", np.linspace(0.1, 0.9, 5))
    return out


def _gene_inputs(p, g, H=None):
    H = p["H"] if H is None else H
    B = basis64(p["phis"], H)
    logm = p["a"] * np.log(p["n"])
    r = None
    if p["noisemodel"] == "NegativeBinomial":
        d = np.asarray(p["dispersion"], dtype=np.float64).reshape(-1)
        r = 1.0 / (d[g] if d.size > 1 else d[0])
    prior = None
    if p["prior"] is not None:
        K = 2 * H + 1
        prior = (p["prior"][0][:K, g], p["prior"][1][:K, g])
    return np.trunc(p["S"][:, g]), B, logm, r, prior


@lru_cache(maxsize=None)
def solved(name):
    """Per gene of a case: (float64 fit, float64 null fit, float32 restatement, its null)."""
    p = cases()[name]
    out = []
    for g in range(p["S"].shape[1]):
        k, B, logm, r, prior = _gene_inputs(p, g)
        k0, B0, _, _, prior0 = _gene_inputs(p, g, 0)
        out.append((newton64(k, B, logm, p["noisemodel"], r, prior), newton64(k0, B0, logm, p["noisemodel"], r, prior0),
                    restate32(k, B, logm, p["noisemodel"], r, prior), restate32(k0, B0, logm, p["noisemodel"], r, prior0)))
    return out


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst distance from float64 over every gene of every case, per yardstick, and the restatement's
    iteration counts per case (name -> list)."""
    worst = dict(coef=0.0, std=0.0, loglik=0.0, lr=0.0)
    for name in cases():
        for (f64, n64, f32, n32) in solved(name):
            d = distances(f32["nu"], f32["std"], f32["loglik"], 2 * (f32["loglik"] - n32["loglik"]), f64, n64)
            for key in worst:
                worst[key] = max(worst[key], d[key])
    return {key: SAFETY * v for key, v in worst.items()}


def chi2_sf_even(x, dof):
    """Survival function of chi-square with an even number of degrees of freedom: exp(-x/2) sum_{j < dof/2} (x/2)^j / j!."""
    x = max(float(x), 0.0) / 2
    return math.exp(-x) * sum(x ** j / math.factorial(j) for j in range(dof // 2)) if dof else 1.0
