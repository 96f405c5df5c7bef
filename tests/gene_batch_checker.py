"""Checker of the batch-aware per-gene harmonic regression (Cycle.from_phases_batch_mle / velocycle_amd.gene_batch / vc_gene_glm_batch):

    eta_c = nu . B[:, c] + delta_b(c) + a log n_c,   mu = exp(eta),   Poisson or negative binomial as in tests/gene_glm_checker.py
    objective   sum_c log p  -  sum_b (delta_b - m_b)^2 / (2 s_b^2)  -  [optional Gaussian prior on nu]

`newton64` is the float64 reference.  It does NOT use the block structure: the batch indicators are K..K+Nb-1 further rows of the design
and the problem is handed to `gene_glm_checker.newton64` (its `eval64` / `logp64`), a dense undamped Newton iteration on the full
(K + Nb) x (K + Nb) penalised system to dec <= 1e-24 max(1, |L|).  `restate32` is a float32 restatement of the device kernel's contract:
the sums of `gene_glm_checker.eval32` on the augmented design (float32 mu, residual, weight and logarithm, float64 sums in another
order), then the step through the Schur complement of the diagonal delta block (`schur`), and the kernel's rules over the K + Nb
coefficients.  Its own distance from float64 over the GPU cases sets the bars (SAFETY x its worst; none is fixed in advance).

Yardsticks: (nu, delta) jointly in standard errors sqrt(d' H64 d) (capped at COEF_CAP); stds of nu and of delta relative; loglik and
lr_stat in units of eps32 sum_c |log p_c| at the float64 optimum."""
from functools import lru_cache

import numpy as np

from tests import gene_glm_checker as G

EPS32, SAFETY, COEF_CAP = G.EPS32, G.SAFETY, G.COEF_CAP
MAX_BATCHES = 32               # VC_GLM_MAX_BATCHES
DELTA_PRIOR = (0.0, 0.5)       # the phase model's muDnu, sigmaDnu


def one_hot(labels, Nb=None):
    labels = np.asarray(labels)
    Nb = int(labels.max()) + 1 if Nb is None else Nb
    return (labels[None, :] == np.arange(Nb)[:, None]).astype(np.float64)          # [Nb, Nc]


def augmented(B, labels, prior, dprior):
    """The design with the batch indicators as trailing rows and the prior of all K + Nb coefficients as (means, stds); a nu
    coefficient without a prior has a NaN mean (gene_glm_checker._prior gives it none)."""
    K = B.shape[0]
    Z = one_hot(labels)
    Nb = Z.shape[0]
    pm = np.full(K, np.nan) if prior is None else np.asarray(prior[0], dtype=np.float64)
    ps = np.ones(K) if prior is None else np.asarray(prior[1], dtype=np.float64)
    dm = np.broadcast_to(np.asarray(dprior[0], dtype=np.float64), (Nb,))
    ds = np.broadcast_to(np.asarray(dprior[1], dtype=np.float64), (Nb,))
    return np.vstack([B, Z]), (np.concatenate([pm, dm]), np.concatenate([ps, ds]))


def newton64(k, B, labels, logm, noisemodel, r=None, prior=None, dprior=DELTA_PRIOR):
    """One gene.  gene_glm_checker.newton64's dict over the K + Nb coefficients (nu first), plus K."""
    Ba, pa = augmented(B, labels, prior, dprior)
    out = G.newton64(k, Ba, logm, noisemodel, r, pa)
    out["K"] = B.shape[0]
    return out


def schur(gsum, Hsum, K, pp, dnu, q, ddelta):
    """The Newton step of the penalised system through the Schur complement of its diagonal delta block, from the UNPENALISED sums
    (gradient gsum and Hessian Hsum over the K + Nb coefficients), the precisions pp [K] and q [Nb] and the distances from the prior
    means dnu = nu - m [K], ddelta = delta - m [Nb].  Row and column 0 of S and entry 0 of the right-hand side are formed without
    cancellation, as the kernel forms them: S_0j = sum_b h_bj q_b / D_b, rhs_0 = sum_b q_b (ddelta_b + g_b / D_b) - pp_0 dnu_0.
    Returns (step [K + Nb], dec, S, D, h); raises LinAlgError when a D_b or a pivot of S is not a positive finite number."""
    h = Hsum[K:, :K]
    D = h[:, 0] + q
    if not (np.isfinite(D).all() and (D > 0).all()):
        raise np.linalg.LinAlgError("D_b")
    g_b = gsum[K:] - q * ddelta
    S = Hsum[:K, :K] + np.diag(pp) - (h / D[:, None]).T @ h
    S[0, :] = S[:, 0] = (h * (q / D)[:, None]).sum(0)
    S[0, 0] += pp[0]
    rhs = gsum[:K] - pp * dnu - h.T @ (g_b / D)
    rhs[0] = (q * (ddelta + g_b / D)).sum() - pp[0] * dnu[0]
    np.linalg.cholesky(S)
    step_nu = np.linalg.solve(S, rhs)
    return np.concatenate([step_nu, (g_b - h @ step_nu) / D]), float(rhs @ step_nu + (g_b * g_b / D).sum()), S, D, h


def restate32(k, B, labels, logm, noisemodel, r=None, prior=None, dprior=DELTA_PRIOR, tol=1e-10, max_iter=25):
    """One gene, the kernel's contract in float32 terms.  Returns dict(nu [K + Nb], cov_nu, std [K + Nb], loglik, dec, iterations, status)."""
    K = B.shape[0]
    Ba, pa = augmented(B, labels, prior, dprior)
    n = Ba.shape[0]
    pm, pp = G._prior(pa, n)
    k32, B32, logm32 = k.astype(np.float32), Ba.astype(np.float32), logm.astype(np.float32)
    r32 = np.float32(r) if r is not None else None
    const = G.constants64(k, noisemodel, float(r32) if r32 is not None else None)
    x = G.start(k, logm32.astype(np.float64), n, pm, pp)
    nan = float("nan")

    def pen(y):
        d = y - pm
        return 0.5 * (pp * d * d).sum()

    e = G.eval32(x, k32, B32, logm32, noisemodel, r32, const)
    status, steps, halvings, dec = G.MAX_ITER, 0, G.HALVINGS, nan
    cov_nu, dvar = np.full((K, K), nan), np.full(n - K, nan)
    while True:
        g = e["grad"] - pp * (x - pm)
        try:
            dx, dec, S, D, h = schur(e["grad"], e["hess"], K, pp[:K], (x - pm)[:K], pp[K:], (x - pm)[K:])
            cov_nu = np.linalg.inv(S)
            dvar = 1.0 / D + np.einsum("bi,ij,bj->b", h, cov_nu, h) / D ** 2
        except np.linalg.LinAlgError:
            status, cov_nu, dvar = G.SINGULAR, np.full((K, K), nan), np.full(n - K, nan)
            break
        if not np.isfinite(dec):
            status = G.SINGULAR
            break
        if dec <= tol:
            status = G.CONVERGED
            break
        if (np.abs(g) <= 4 * EPS32 * np.sqrt(e["N"])).all():
            status = G.ROUNDING
            break
        if steps >= max_iter:
            break
        t, moved = 1.0, False
        while True:
            trial = x + t * dx
            if np.abs(trial[1:]).max(initial=0.0) > G.BOUND:
                status = G.UNBOUNDED
                break
            e2 = G.eval32(trial, k32, B32, logm32, noisemodel, r32, const)
            if e2["L"] - pen(trial) >= e["L"] - pen(x) - 8 * EPS32 * max(e["A"], e2["A"]):
                x, e, moved = trial, e2, True
                break
            if halvings == 0:
                break
            halvings -= 1
            t *= 0.5
        if not moved:
            break
        steps += 1
    return dict(nu=x, K=K, cov_nu=cov_nu, std=np.sqrt(np.concatenate([np.diag(cov_nu), dvar])), loglik=e["loglik"], dec=dec,
                iterations=steps, status=status)


def distances(got_nu, got_delta, got_std, got_dstd, got_ll, got_lr, ref, ref_null):
    """The five yardsticks of one gene against its float64 fits (full model `ref`, constant plus offsets `ref_null`)."""
    K = ref["K"]
    d = np.concatenate([np.asarray(got_nu, dtype=np.float64), np.asarray(got_delta, dtype=np.float64)]) - ref["nu"]
    scale = EPS32 * ref["abs"]
    return dict(coef=float(np.sqrt(max(d @ ref["hess"] @ d, 0.0))), std=float(np.abs(np.asarray(got_std) / ref["std"][:K] - 1).max()),
                dstd=float(np.abs(np.asarray(got_dstd) / ref["std"][K:] - 1).max()), loglik=float(abs(got_ll - ref["loglik"]) / scale),
                lr=float(abs(got_lr - 2 * (ref["loglik"] - ref_null["loglik"])) / scale))


# ---------------------------------------------------------------------------------------------------------------------------------
# The problems of tests/test_hip_gene_batch.py, built once and shared with tests/test_gene_batch_cpu.py.

SEVEN = (1, 63, 64, 65, 255, 256, 257)
NOISES = G.NOISES


@lru_cache(maxsize=None)
def simulated(sizes, Ng, seed=1, level=1.5, thirds=False, dnu_std=0.5):
    """Batches of the given sizes, cells in batch order: S [Nc, Ng] negative-binomial counts (shape_inv 0.3) at
    mu = exp(nu . zeta(phi) + dnu[b]), n = 1 for every cell.  thirds: batch b covers the b-th part of the cycle only."""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    Nc, Nb = labels.size, len(sizes)
    phis = rng.uniform(0, 2 * np.pi, Nc)
    if thirds:
        phis = (labels + rng.uniform(0, 1, Nc)) * 2 * np.pi / Nb
    nu = np.vstack([rng.uniform(level - 1.0, level + 1.0, Ng), rng.normal(0, 0.4, (2, Ng))])          # [3, Ng]
    dnu = rng.normal(0, dnu_std, (Nb, Ng))
    mu = np.exp(G.basis64(phis, 1).T @ nu + dnu[labels])
    S = rng.poisson(rng.gamma(1 / 0.3, 0.3 * mu)).astype(np.float64)
    return dict(S=S, phis=phis, labels=labels, n=np.ones(Nc), nu=nu, dnu=dnu)


def problem(S, phis, n, labels, H, noisemodel, dispersion=None, prior=None, dprior=DELTA_PRIOR):
    return dict(S=np.asarray(S, dtype=np.float64), phis=np.asarray(phis, dtype=np.float64), n=np.asarray(n, dtype=np.float64),
                labels=np.asarray(labels), H=H, noisemodel=noisemodel, dispersion=dispersion, prior=prior, dprior=dprior, a=1.0)


def large(extra=None):
    """Three batches of a (257, 2) problem with counts around 2e4; extra: a count that replaces the first of gene 0 (70 000: float32)."""
    sim = simulated((100, 57, 100), 2, seed=3, level=10.0)
    S = sim["S"].copy()
    if extra is not None:
        S[0, 0] = extra
    return S, sim["phis"], sim["n"], sim["labels"]


def separated():
    """gene_glm_checker.separated() with its 257 cells in three batches."""
    S, phis, n = G.separated()
    return S, phis, n, np.repeat(np.arange(3), (100, 57, 100))


@lru_cache(maxsize=None)
def cases():
    """name -> problem: every problem the GPU tests hold against the bars."""
    out = {}
    sim = simulated(SEVEN, 5)
    for H in (0, 1, 2):
        for noise, disp in NOISES:
            out[f"seven_{H}_{noise}"] = problem(sim["S"], sim["phis"], sim["n"], sim["labels"], H, noise, disp)
    sim = simulated((257,), 3, seed=2)
    out["one_batch"] = problem(sim["S"], sim["phis"], sim["n"], sim["labels"], 1, "NegativeBinomial", 0.3)
    sim = simulated((1, 1000), 3, seed=4)
    out["one_and_1000"] = problem(sim["S"], sim["phis"], sim["n"], sim["labels"], 1, "Poisson")
    sim = simulated((8,) * MAX_BATCHES, 3, seed=5)
    out["max_batches"] = problem(sim["S"], sim["phis"], sim["n"], sim["labels"], 1, "NegativeBinomial", 0.3)
    sim = simulated((100, 100, 100), 4, seed=6)
    order = np.random.default_rng(6).permutation(300)                                # interleaved labels: the worker has to sort
    out["interleaved"] = problem(sim["S"][order], sim["phis"][order], sim["n"], sim["labels"][order], 1, "Poisson")
    S = sim["S"].copy()
    S[100:200, 0] = 0.0                                                              # gene 0 has no count in the whole of batch 1
    out["silent_batch"] = problem(S, sim["phis"], sim["n"], sim["labels"], 1, "NegativeBinomial", 0.3)
    for noise, disp in NOISES:
        out[f"large_u16_{noise}"] = problem(*large(), 1, noise, disp)
        out[f"large_f32_{noise}"] = problem(*large(70000.0), 1, noise, disp)
    out["nu_prior"] = problem(sim["S"], sim["phis"], sim["n"], sim["labels"], 1, "NegativeBinomial", np.linspace(0.2, 0.5, 4),
                              (np.zeros((3, 4)), np.vstack([np.full((1, 4), 10.0), np.ones((2, 4))])),
                              (np.linspace(-0.2, 0.2, 12).reshape(3, 4), np.linspace(0.3, 0.8, 12).reshape(3, 4)))
    return out


def gene_inputs(p, g, H=None):
    H = p["H"] if H is None else H
    B = G.basis64(p["phis"], H)
    logm = p["a"] * np.log(p["n"])
    r = None
    if p["noisemodel"] == "NegativeBinomial":
        d = np.asarray(p["dispersion"], dtype=np.float64).reshape(-1)
        r = 1.0 / (d[g] if d.size > 1 else d[0])
    prior = None
    if p["prior"] is not None:
        K = 2 * H + 1
        prior = (p["prior"][0][:K, g], p["prior"][1][:K, g])
    dprior = tuple(np.asarray(v, dtype=np.float64)[:, g] if np.ndim(v) == 2 else v for v in p["dprior"])
    return np.trunc(p["S"][:, g]), B, p["labels"], logm, r, prior, dprior


@lru_cache(maxsize=None)
def solved(name):
    """Per gene of a case: (float64 fit, float64 null fit, float32 restatement, its null); the null is K = 1 with the offsets."""
    p = cases()[name]
    out = []
    for g in range(p["S"].shape[1]):
        k, B, lab, logm, r, prior, dprior = gene_inputs(p, g)
        _, B0, _, _, _, prior0, _ = gene_inputs(p, g, 0)
        out.append((newton64(k, B, lab, logm, p["noisemodel"], r, prior, dprior), newton64(k, B0, lab, logm, p["noisemodel"], r, prior0, dprior),
                    restate32(k, B, lab, logm, p["noisemodel"], r, prior, dprior), restate32(k, B0, lab, logm, p["noisemodel"], r, prior0, dprior)))
    return out


YARDSTICKS = ("coef", "std", "dstd", "loglik", "lr")


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst distance from float64 over every gene of every case, per yardstick."""
    worst = dict.fromkeys(YARDSTICKS, 0.0)
    for name in cases():
        for (f64, n64, f32, n32) in solved(name):
            K = f64["K"]
            d = distances(f32["nu"][:K], f32["nu"][K:], f32["std"][:K], f32["std"][K:], f32["loglik"], 2 * (f32["loglik"] - n32["loglik"]),
                          f64, n64)
            for key in worst:
                worst[key] = max(worst[key], d[key])
    return {key: SAFETY * v for key, v in worst.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# The container round trip: 600 cells x 30 genes, three batches that cover different thirds of the cycle, known offsets.

ROUND_TRIP_SEED = 11


@lru_cache(maxsize=None)
def round_trip():
    return simulated((200, 200, 200), 30, seed=ROUND_TRIP_SEED, level=2.0, thirds=True)


def single_sample_bias(sim):
    """max over genes of |true sin / cos coefficient - single-sample float64 fit| in that fit's own standard errors."""
    B, logm = G.basis64(sim["phis"], 1), np.log(sim["n"])
    worst = 0.0
    for g in range(sim["S"].shape[1]):
        fit = G.newton64(sim["S"][:, g], B, logm, "NegativeBinomial", 1 / 0.3)
        worst = max(worst, float(np.abs((fit["nu"][1:] - sim["nu"][1:, g]) / fit["std"][1:]).max()))
    return worst
