"""Checker of the weighted joint fit (vc_gene_joint_weighted, `velocycle_amd.joint_bootstrap.gene_joint_weighted`) and of the cell
bootstrap of its MAP angular speed (`velocity_map_joint_bootstrap`).  It holds no weighted formula for integer weights: a fit under
integer case weights IS the unweighted fit of the data with every cell repeated w_c times, so the float64 reference of a (row, gene) pair
is tests/gene_joint_checker.py's `solve64` on `np.repeat` of S, U, phis, n and the columns of W, and the float32 restatement its `solve32`
on the same expansion: from the bootstrap's warm start (the float64 fit of the unweighted data) and from the default start.  The outer
reference and restatement are `gene_joint_checker._outer`'s rules, written out here in a variant that takes first-round starts
(`outer_from`: `_outer` itself begins with starts=None).  Bars are formed as `Q.bars()` forms them: Q.SAFETY x the restatement's worst
distance from float64 over these cases, on Q's yardsticks; never from the code under test.

Non-integer weights have `weighted_point64` / `weighted_solve64`, written out from the formulas (wt the cell's weight):

    res, w, wo of both layers -> wt res, wt w, wt wo in G, O, F, the score and the information;   L_S, L_U = sum wt log p;
    A = sum wt |terms|;   N_i = sum ((wt woS)^2 + (wt resS)^2) gS_i^2 + ((wt woU)^2 + (wt resU)^2) gU_i^2;
    n_clamped = #{w > 0, z <= 0};   default start nu_0 = ln(sum wt k_S / sum wt e^logm), y = ln(sum wt e^etaS zp / sum wt k_U);
    the priors unweighted.

Weights are Poisson(1) draws of `np.random.default_rng(seed).poisson(1, (rows, Nc))`.  WARM_SEED = 22: with it every pair of all 18
cases is kink-free (min z >= MIN_Z at every point the reference evaluates, refused trials included) and CONVERGED from the warm start
(seed 11, the kinetics checker's, clamps one pair of score_257_5_2).  From the default start the first full step of three cases runs
into the kink for every seed in 11..40; the others use the first seed of that range for which every pair of the case is kink-free
(DEFAULT_SEEDS).  A row that leaves a gene without a weighted count in a layer has no fit (NO_DATA): `left_out` names those pairs."""
import math
from functools import lru_cache

import numpy as np

from tests import gene_joint_checker as Q
from tests.gene_kinetics_checker import OUTER_HALVINGS, nuw_prior

WARM_SEED = 22
ROWS, OUTER_ROWS = 3, 2
PAIR_CASES = Q.FIT_CASES + Q.SCORE_CASES
DEFAULT_SEEDS = {"shape_1_1_1_Poisson": 11, "shape_63_2_2_NegativeBinomial": 11, "shape_64_3_1_NegativeBinomial": 11,
                 "shape_1025_3_1_Poisson": 11, "shape_1025_3_2_NegativeBinomial": 11, "large_u16": 11, "score_257_5_1": 11,
                 "score_257_5_3": 11, "score_1025_3_2": 11, "large_f32": 12, "score_1025_3_3": 12, "shape_256_1_2_NegativeBinomial": 16,
                 "shape_257_5_1_NegativeBinomial": 16, "score_1025_3_1": 16, "shape_255_5_1_Poisson": 31}
NO_DEFAULT_TOLERANCE = ("shape_65_4_2_Poisson", "shape_257_5_2_Poisson", "score_257_5_2")     # no kink-free seed in 11..40
UNIFORM_CASE = "shape_257_5_1_NegativeBinomial"


def weights(name, seed=WARM_SEED, rows=ROWS):
    """float64 [rows, Nc]: the Poisson(1) resamples of a case."""
    return np.random.default_rng(seed).poisson(1, (rows, Q.cases()[name]["U"].shape[0])).astype(np.float64)


def uniform_weights():
    """float64 [2, 257] holding float32 values (the table is float32 by contract), uniform on (0, 3)."""
    return np.random.default_rng(WARM_SEED).uniform(0, 3, (2, 257)).astype(np.float32).astype(np.float64)


def expand(p, w):
    """The problem with cell c repeated w_c times (integer weights)."""
    w = np.asarray(w)
    reps = w.astype(np.int64)
    assert np.array_equal(reps, w), "integer weights only"
    out = dict(p, S=np.repeat(p["S"], reps, axis=0), U=np.repeat(p["U"], reps, axis=0), phis=np.repeat(p["phis"], reps),
               n=np.repeat(p["n"], reps), W=np.repeat(p["W"], reps, axis=1))
    if p.get("D") is not None:
        out["D"] = np.repeat(p["D"], reps, axis=1)
    return out


def has_data(p, w, g):
    w = np.asarray(w)
    return float((w * p["S"][:, g]).sum()) > 0 and float((w * p["U"][:, g]).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- non-integer weights
def weighted_point64(th, kS, kU, B, logm, W, nuw, wt, noisemodel, r=None, prior=None):
    """The formulas of the module's docstring at theta, float64.  The keys are those of `Q.point64`."""
    th = np.asarray(th, dtype=np.float64)
    wt = np.asarray(wt, dtype=np.float64)
    K, Nc = B.shape
    D = K + 2
    pm, pp = Q.prior_of(K) if prior is None else prior
    nu, x, y = th[:K], th[K], th[K + 1]
    dB = Q.db_from_basis(B)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d, om, ex = nu @ dB, nuw @ W, math.exp(x)
        z = om * d + ex
        a = z > 0
        zp = np.where(a, z, 0.0) + Q.FLOOR
        etaS = nu @ B + logm
        etaU = etaS - y + np.log(zp)
        (rS, wS, oS), lpS, partsS = Q._lik64(kS, etaS, noisemodel, r)
        (rU, wU, oU), lpU, partsU = Q._lik64(kU, etaU, noisemodel, r)
        rS, wS, oS, rU, wU, oU = (wt * v for v in (rS, wS, oS, rU, wU, oU))
        p, s, q = np.where(a, ex / zp, 0.0), np.where(a, om / zp, 0.0), np.where(a, d / zp, 0.0)
        gS = np.concatenate([B, np.zeros((2, Nc))])
        gU = np.concatenate([B + s * dB, p[None], -np.ones((1, Nc))])
        u = np.concatenate([s * dB, p[None], np.zeros((1, Nc))])
        outer = lambda v, c: (c * v[:, None, :] * v[None, :, :]).sum(-1)                # noqa: E731
        G = (rS * gS).sum(-1) + (rU * gU).sum(-1) - pp * (th - pm)
        O = outer(gS, oS) + outer(gU, oU) + outer(u, rU) + np.diag(pp)
        O[K, K] -= (rU * p).sum()
        F = outer(gS, wS) + outer(gU, wU) + np.diag(pp)
        observed = Q._chol_ok(O)
        M = O if observed else F
        inv = np.linalg.inv(M)
        step = inv @ G
        L_S, L_U = float((wt * lpS).sum()), float((wt * lpU).sum())
        pen = 0.5 * float((pp * (th - pm) ** 2).sum())
        qW = q[None, :] * W
        NW = W.shape[0]
        Iww = (wU[None, None, :] * qW[:, None, :] * qW[None, :, :]).sum(-1)
        Iwt = (wU[None, None, :] * qW[:, None, :] * gU[None, :, :]).sum(-1).reshape(NW, D)
        on = wt > 0
        return dict(th=th, L_S=L_S, L_U=L_U, L=L_S + L_U, A=float((wt * (partsS + partsU)).sum()), f=L_S + L_U - pen, G=G, M=M, O=O, F=F,
                    observed=observed, inv=inv, step=step, dec=float(G @ step), fisher_step=np.linalg.solve(F, G),
                    N=((oS * oS + rS * rS) * gS * gS).sum(-1) + ((oU * oU + rU * rU) * gU * gU).sum(-1), n_clamped=int((on & ~a).sum()),
                    score=(rU * qW).sum(-1), info=Iww - Iwt @ np.linalg.inv(F) @ Iwt.T,
                    score_unit=4 * Q.EPS32 * np.sqrt(((wU * wU + rU * rU) * qW ** 2).sum(-1)),
                    abs_S=float((wt * np.abs(lpS)).sum()), abs_U=float((wt * np.abs(lpU)).sum()),
                    minz=float(np.where(a, zp - Q.FLOOR, -1.0)[on].min()) if on.any() else math.inf)


def weighted_start(kS, kU, B, logm, W, nuw, wt, prior):
    K = B.shape[0]
    th = prior[0].copy()
    th[0] = math.log((wt * kS).sum() / (wt * np.exp(logm)).sum())
    z = (nuw @ W) * (th[:K] @ Q.db_from_basis(B)) + math.exp(th[K])
    zp = np.where(z > 0, z, 0.0) + Q.FLOOR
    th[K + 1] = math.log((wt * np.exp(th[:K] @ B + logm) * zp).sum() / (wt * kU).sum())
    return np.clip(th, -Q.bounds(K), Q.bounds(K))


def weighted_solve64(kS, kU, B, logm, W, nuw, wt, noisemodel, r=None, prior=None, start=None, max_iter=80):
    """`Q.solve64`'s iteration on `weighted_point64`."""
    prior = Q.prior_of(B.shape[0]) if prior is None else prior
    pt = lambda th: weighted_point64(th, kS, kU, B, logm, W, nuw, wt, noisemodel, r, prior)      # noqa: E731
    th = Q._start(start, weighted_start(kS, kU, B, logm, W, nuw, wt, prior), B.shape[0])
    return Q._iterate(pt, th, lambda e: 1e-24 * max(1.0, abs(e["f"])), max_iter, Q.EPS64, False)


# ---------------------------------------------------------------------------------------------------------------- the pairs
def _solve_pair(p, w, g, start):
    """(reference, restatement) of gene g under the integer weights w, both from `start` (None: the default start)."""
    pe = expand(p, w)
    kS, kU, B, logm, r = Q.gene_inputs(pe, g)
    args = (kS, kU, B, logm, pe["W"], p["nuw"], p["noisemodel"], r)
    return Q.solve64(*args, start=start), Q.solve32(*args, start=start)


def warm_starts(name):
    """[gene] the float64 fit of the unweighted data: the bootstrap's own start."""
    return [f64["th"] for f64, _ in Q.solved(name)]


@lru_cache(maxsize=None)
def solved_warm(name):
    """[row][gene] of a case under `weights(name)` from the warm start: (reference, restatement), or None where the row leaves a layer
    of the gene without a count."""
    p, starts = Q.cases()[name], warm_starts(name)
    return [[_solve_pair(p, w, g, starts[g]) if has_data(p, w, g) else None for g in range(p["U"].shape[1])] for w in weights(name)]


@lru_cache(maxsize=None)
def solved_default(name):
    """The same from the default start, under `weights(name, DEFAULT_SEEDS[name])`."""
    p = Q.cases()[name]
    return [[_solve_pair(p, w, g, None) if has_data(p, w, g) else None for g in range(p["U"].shape[1])]
            for w in weights(name, DEFAULT_SEEDS[name])]


def left_out(solved, names):
    """{(case, row, gene)} of the pairs without a weighted count in a layer."""
    return {(name, b, g) for name in names for b, row in enumerate(solved(name)) for g, s in enumerate(row) if s is None}


def assert_kink_free(name, rows):
    """Every pair of a tolerance-bearing case: min z >= MIN_Z at every point the reference visits, and the reference CONVERGED."""
    for b, row in enumerate(rows):
        for g, s in enumerate(row):
            if s is not None:
                assert s[0]["minz_path"] >= Q.MIN_Z and s[0]["status"] == Q.CONVERGED, (name, b, g, s[0]["minz_path"], s[0]["status"])


@lru_cache(maxsize=None)
def solved_uniform():
    """[row][gene] of UNIFORM_CASE under `uniform_weights()` from the warm start: the reference of the written-out formulas (no
    restatement; from the default start the first full step of this case runs into the kink)."""
    p = Q.cases()[UNIFORM_CASE]
    starts = warm_starts(UNIFORM_CASE)
    out = []
    for w in uniform_weights():
        row = []
        for g in range(p["U"].shape[1]):
            kS, kU, B, logm, r = Q.gene_inputs(p, g)
            row.append(weighted_solve64(kS, kU, B, logm, p["W"], p["nuw"], w, p["noisemodel"], r, start=starts[g]))
        out.append(row)
    return out


@lru_cache(maxsize=None)
def evaluated():
    """{(row, i, g): (reference, restatement, theta)} at Q.EVALUATE_AT[i] of Q.EVALUATE_CASE under its weights; the point None is the
    weighted default start (the unweighted one of the expansion)."""
    p = Q.cases()[Q.EVALUATE_CASE]
    out = {}
    for b, w in enumerate(weights(Q.EVALUATE_CASE)):
        pe = expand(p, w)
        for g in range(p["U"].shape[1]):
            kS, kU, B, logm, r = Q.gene_inputs(pe, g)
            for i, th in enumerate(Q.evaluate_points(pe, g)):
                out[(b, i, g)] = (Q.point64(th, kS, kU, B, logm, pe["W"], p["nuw"], p["noisemodel"], r),
                                  Q.point32(th, kS, kU, B, logm, pe["W"], p["nuw"], p["noisemodel"], r), th)
    return out


# ---------------------------------------------------------------------------------------------------------------- the outer fit
def outer_from(p, solve, ok, tol_outer, max_rounds, allowance, nuw0, starts0, trace=None):
    """`Q._outer`'s rules with the first round's genes started at starts0[g] (the bootstrap's warm start)."""
    Ng = p["U"].shape[1]
    pm, pp = nuw_prior(p["Nx"], p["Hw"])
    genes = [Q.gene_inputs(p, g) for g in range(Ng)]

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

    v = np.asarray(nuw0, dtype=np.float64)
    cur = evaluate(v, starts0, None)
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


@lru_cache(maxsize=None)
def outer_solved(name):
    """[row] of an outer case under its 2 rows: (reference, restatement, the reference's trace), both started at the reference's
    full-data angular speed and genes (the bootstrap's warm start)."""
    from tests.gene_kinetics_checker import MAX_ROUNDS, TOL_OUTER
    p = Q.cases()[name]
    full = Q.outer_solved(name)[0]
    starts = [f["th"] for f in full["fits"]]
    out = []
    for w in weights(name, rows=OUTER_ROWS):
        pe, trace = expand(p, w), []
        m64 = outer_from(pe, Q.solve64, lambda f: f["status"] == Q.CONVERGED, 1e-14, 60, 8 * Q.EPS64, full["nuw"], starts, trace)
        m32 = outer_from(pe, Q.solve32, lambda f: f["status"] in Q.INTERIOR, TOL_OUTER, MAX_ROUNDS, 8 * Q.EPS32, full["nuw"], starts)
        out.append((m64, m32, trace))
    return out


# ---------------------------------------------------------------------------------------------------------------- bars
def _pair_worst(w, name, p, rows, wts):
    steps = 0
    for b, row in enumerate(rows):
        pe = expand(p, wts[b])
        for g, s in enumerate(row):
            if s is None:
                continue
            f64, f32 = s
            assert f64["status"] == Q.CONVERGED and f32["status"] in Q.INTERIOR, (name, b, g, f64["status"], f32["status"])
            steps = max(steps, f32["iterations"])
            w["theta"] = max(w["theta"], Q.theta_distance(f32["th"], f64))
            w["cov"] = max(w["cov"], Q.sym_distance(f32["inv"], f64["inv"]))
            key = "loglik_large" if name in Q.LARGE_CASES else "loglik"
            w[key] = max(w[key], Q.loglik_distance(f32["L_S"], f64, "S"), Q.loglik_distance(f32["L_U"], f64, "U"))
            if name in Q.SCORE_CASES:
                w["info"] = max(w["info"], Q.sym_distance(f32["info"], f64["info"]))
                kS, kU, B, logm, r = Q.gene_inputs(pe, g)            # the score at the SAME point: the reference's optimum
                at = Q.point32(f64["th"], kS, kU, B, logm, pe["W"], p["nuw"], p["noisemodel"], r)
                w["score"] = max(w["score"], Q.score_distance(at["score"], f64))
    return steps


@lru_cache(maxsize=None)
def bars():
    """Q.SAFETY x the restatement's worst distance from the reference over the pairs of PAIR_CASES from the warm start, the
    DEFAULT_SEEDS cases from the default start, the evaluate-only points and the outer cases, per asserted figure (the keys of
    `Q.bars()`); `steps_warm`, `steps_default`: the restatement's worst number of steps per pair (not multiplied)."""
    w = dict(theta=0.0, cov=0.0, loglik=0.0, loglik_large=0.0, ev_loglik=0.0, ev_dec=0.0, score=0.0, info=0.0, nuw=0.0, std=0.0)
    steps_warm = steps_default = 0
    for name in PAIR_CASES:
        rows = solved_warm(name)
        assert_kink_free(name, rows)
        steps_warm = max(steps_warm, _pair_worst(w, name, Q.cases()[name], rows, weights(name)))
    for name in DEFAULT_SEEDS:
        rows = solved_default(name)
        assert_kink_free(name, rows)
        steps_default = max(steps_default, _pair_worst(w, name, Q.cases()[name], rows, weights(name, DEFAULT_SEEDS[name])))
    for ref, f32, _ in evaluated().values():
        w["ev_loglik"] = max(w["ev_loglik"], Q.loglik_distance(f32["L_S"], ref, "S"), Q.loglik_distance(f32["L_U"], ref, "U"))
        w["ev_dec"] = max(w["ev_dec"], Q.dec_distance(f32["dec"], ref))
    for name in Q.OUTER_CASES:
        for m64, m32, _ in outer_solved(name):
            d = m32["nuw"] - m64["nuw"]
            w["nuw"] = max(w["nuw"], float(math.sqrt(d @ m64["J"] @ d)))
            w["std"] = max(w["std"], float(np.abs(m32["std"] / m64["std"] - 1).max()))
    out = {key: Q.SAFETY * v for key, v in w.items()}
    out["steps_warm"], out["steps_default"] = steps_warm, steps_default
    return out
