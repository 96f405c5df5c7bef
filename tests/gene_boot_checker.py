"""Checker of the weighted per-gene harmonic regression (vc_gene_glm_weighted / velocycle_amd.gene_bootstrap / gene_harmonics with
cell_weights).  It holds no weighted formula for integer weights: a fit under integer case weights IS the unweighted fit of the data with
every cell repeated w_c times, so the float64 reference of a (gene, row) pair is tests/gene_glm_checker.py's `newton64` on
`np.repeat` of k, B and logm, and the float32 restatement its `restate32` on the same expansion.  Bars are formed as `G.bars()` forms
them: G.SAFETY x the restatement's worst distance from float64 over these cases, run from the default start and from the bootstrap's
warm start (the unweighted fit) as the GPU test runs them, on `G.distances`' yardsticks (coefficients
sqrt(d' H64 d) in standard errors; stds |std / std64 - 1|; loglik and lr_stat over eps32 sum_c w_c |log p_c|).

Non-integer weights have `weighted_newton64`, written out from the formulas:

    gradient sum_c w_c res_c B_i,  Hessian sum_c w_c wo_c B_i B_j,  log-likelihood sum_c w_c log p_c,  start nu_0 = ln(sum w k / sum w n^a),
    the prior unweighted; the stopping rule is newton64's.

A resample can separate a sparse gene (its weighted counts sit in too few cells for a finite maximum): the tolerance-bearing pairs are
those whose float64 reference ends CONVERGED; tests/test_gene_bootstrap_cpu.py bounds the share that is left out."""
from contextlib import contextmanager
from functools import lru_cache

import numpy as np

from tests import gene_glm_checker as G

WEIGHT_SEED = 11
SHAPES = [(63, 1, 1), (65, 7, 3), (257, 5, 1), (255, 5, 2), (1000, 3, 3)]
UNIFORM_CASE = "uniform_257_5_1_NegativeBinomial"


def expand(k, B, logm, w):
    """The data with cell c repeated w_c times (integer weights)."""
    w = np.asarray(w)
    reps = w.astype(np.int64)
    assert np.array_equal(reps, w), "integer weights only"
    return np.repeat(k, reps), np.repeat(B, reps, axis=1), np.repeat(logm, reps)


def weighted_newton64(k, B, logm, w, noisemodel, r=None, prior=None, max_iter=60):
    """One gene under float64 case weights w [Nc].  Returns what `G.newton64` returns."""
    K = B.shape[0]
    pm, pp = G._prior(prior, K)
    nu = np.zeros(K) if pm is None else np.where(pp > 0, pm, 0.0)
    nu[0] = np.log((w * k).sum() / (w * np.exp(logm)).sum())
    status = G.MAX_ITER
    for it in range(max_iter + 1):
        eta = nu @ B + logm
        mu = np.exp(eta)
        res, wo = (k - mu, mu) if noisemodel == "Poisson" else ((k - mu) * r / (r + mu), mu * r * (k + r) / (r + mu) ** 2)
        lp = G.logp64(k, eta, noisemodel, r)
        grad, hess, obj = B @ (w * res), (B * (w * wo)) @ B.T, (w * lp).sum()
        if pm is not None:
            d = nu - pm
            grad, hess, obj = grad - pp * d, hess + np.diag(pp), obj - 0.5 * (pp * d * d).sum()
        try:
            step = np.linalg.solve(hess, grad)
            np.linalg.cholesky(hess)
        except np.linalg.LinAlgError:
            status = G.SINGULAR
            break
        dec = float(grad @ step)
        if not np.isfinite(dec):
            status = G.SINGULAR
            break
        if dec <= 1e-24 * max(1.0, abs(obj)):
            status = G.CONVERGED
            break
        if it == max_iter:
            break
        nu = nu + step
        if np.abs(nu[1:]).max(initial=0.0) > G.BOUND:
            status = G.UNBOUNDED
            break
    cov = np.linalg.inv(hess) if status == G.CONVERGED else np.full((K, K), np.nan)
    return dict(nu=nu, hess=hess, cov=cov, std=np.sqrt(np.diag(cov)), loglik=float((w * lp).sum()), abs=float((w * np.abs(lp)).sum()),
                dec=dec, iterations=it, status=status)


@contextmanager
def _starting_at(nu):
    """`G.restate32` has no start argument: it asks `G.start`.  Within this block that answer is `nu`, so that the restatement of a
    warm-started fit is the same existing code run from the warm start."""
    default = G.start
    G.start = lambda *args: np.array(nu, dtype=np.float64)
    try:
        yield
    finally:
        G.start = default


@lru_cache(maxsize=None)
def cases():
    """name -> (problem of tests/gene_glm_checker.py, weights float64 [R, Nc])."""
    base = G.cases()
    out = {}
    for (Nc, Ng, H) in SHAPES:
        w = np.random.default_rng(WEIGHT_SEED).poisson(1, (5, Nc)).astype(np.float64)
        for noise, _ in G.NOISES:
            out[f"shape_{Nc}_{Ng}_{H}_{noise}"] = (base[f"shape_{Nc}_{Ng}_{H}_{noise}"], w)
    w = np.random.default_rng(WEIGHT_SEED).poisson(1, (2, 257)).astype(np.float64)
    for noise, _ in G.NOISES:
        out[f"large_u16_{noise}"] = (base[f"large_u16_{noise}"], w)
        out[f"large_f32_{noise}"] = (base[f"large_f32_{noise}"], w)
    out["prior_wide"] = (base["prior_wide"], w)
    uniform = np.random.default_rng(WEIGHT_SEED).uniform(0, 3, (2, 257)).astype(np.float32)      # the table is float32 by contract
    out[UNIFORM_CASE] = (base["shape_257_5_1_NegativeBinomial"], uniform.astype(np.float64))
    return out


def is_integer(name):
    w = cases()[name][1]
    return bool(np.array_equal(w, np.round(w)))


@lru_cache(maxsize=None)
def solved(name):
    """[row][gene] of a case: (float64 fit, float64 null fit, float32 restatement from the default start, its null, the restatement
    warm-started from the float64 fit of the unweighted data -- the bootstrap's start; the null model is never warm-started); the
    restatements are None under non-integer weights."""
    p, W = cases()[name]
    out = []
    for w in W:
        row = []
        for g in range(p["S"].shape[1]):
            k, B, logm, r, prior = G._gene_inputs(p, g)
            k0, B0, _, _, prior0 = G._gene_inputs(p, g, 0)
            if is_integer(name):
                ke, Be, le = expand(k, B, logm, w)
                _, B0e, _ = expand(k0, B0, logm, w)
                with _starting_at(G.newton64(k, B, logm, p["noisemodel"], r, prior)["nu"]):
                    warm = G.restate32(ke, Be, le, p["noisemodel"], r, prior)
                row.append((G.newton64(ke, Be, le, p["noisemodel"], r, prior), G.newton64(ke, B0e, le, p["noisemodel"], r, prior0),
                            G.restate32(ke, Be, le, p["noisemodel"], r, prior), G.restate32(ke, B0e, le, p["noisemodel"], r, prior0), warm))
            else:
                row.append((weighted_newton64(k, B, logm, w, p["noisemodel"], r, prior),
                            weighted_newton64(k0, B0, logm, w, p["noisemodel"], r, prior0), None, None, None))
        out.append(row)
    return out


def bearing(name):
    """bool [R, Ng]: the pairs held to the bars (their float64 reference, and its null model, end CONVERGED)."""
    return np.array([[s[0]["status"] == G.CONVERGED and s[1]["status"] == G.CONVERGED for s in row] for row in solved(name)])


@lru_cache(maxsize=None)
def bars():
    """G.SAFETY x the restatement's worst distance from float64 over every tolerance-bearing pair of every integer-weight case, from
    both starts the GPU test runs.  The warm start matters to the stds: a fit ends wherever its decrement first falls under tol, that
    is anywhere within sqrt(tol) = 1e-5 standard errors of the optimum, and the Hessian there differs by that distance times the
    likelihood's skewness, which is of order one in the nearly separated pairs of (65, 7, 3).  From the default start the last Newton
    step usually lands far below tol; from the warm start it need not (restatement: 5.6e-6 against 6.2e-7 on the stds)."""
    worst = dict(coef=0.0, std=0.0, loglik=0.0, lr=0.0)
    for name in cases():
        if not is_integer(name):
            continue
        keep = bearing(name)
        for b, row in enumerate(solved(name)):
            for g, (f64, n64, f32, n32, f32w) in enumerate(row):
                if keep[b, g]:
                    for f in (f32, f32w):
                        d = G.distances(f["nu"], f["std"], f["loglik"], 2 * (f["loglik"] - n32["loglik"]), f64, n64)
                        for key in worst:
                            worst[key] = max(worst[key], d[key])
    return {key: G.SAFETY * v for key, v in worst.items()}


def iteration_bound(name, b, g, warm=False):
    """The steps a device fit of the pair may take: the restatement's from the same start + 2; under non-integer weights (no
    restatement) the float64 Newton's + 2 -- it runs undamped from the default start to a decrement of 1e-24, far below the device's
    tol, and the warm start is nearer to the optimum than the default one."""
    f64, _, f32, _, f32w = solved(name)[b][g]
    return ((f32w if warm else f32) if f32 is not None else f64)["iterations"] + 2
