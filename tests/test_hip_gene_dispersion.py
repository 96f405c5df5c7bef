"""GPU: vc_gene_dispersion through `gene_dispersion`, the joint fit `gene_harmonics(dispersion="mle")` and the loop
`Cycle.from_phases_mle(dispersion="mle")` -> `Phases.from_cycle_mle`, held to the reference and the bars of
tests/gene_dispersion_checker.py.  Every test prints the figures it asserts on."""
import math
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch
from scipy.special import gammaln

from tests import gene_dispersion_checker as D
from tests import gene_glm_checker as G
from tests.test_gene_dispersion_cpu import REFUSALS, disp_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.gene_harmonics import MLE_FIELDS, GeneHarmonicFit, gene_dispersion, gene_harmonics

pytestmark = pytest.mark.gpu


def run(name, **kw):
    p = D.cases()[name]
    return gene_dispersion(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], p["nu"].T, prior=p["prior"], **kw)


def bound_r32(status):
    return np.float32(math.exp(D.RHO_MAX if status == D.AT_UPPER else D.RHO_MIN))


def assert_within_bars(name, fit):
    bars, worst = D.bars(), dict(rho=0.0, std=0.0)
    for g, (f64, f32) in enumerate(D.solved(name)):
        if f64["status"] == D.CONVERGED:
            assert fit.status[g] in D.INTERIOR, (name, g, fit.status[g])
            d = D.fit_distances(fit.log_r[g], fit.log_r_std[g], f64)
            worst = {key: max(worst[key], d[key]) for key in worst}
            assert fit.dispersion[g] == 1.0 / float(np.float32(math.exp(fit.log_r[g])))
            assert abs(fit.score[g]) <= max(math.sqrt(D.TOL * f64["info"]) * 1.01, f32["noise"] * 1.01)
        else:
            assert fit.status[g] == f64["status"], (name, g, fit.status[g], f64["status"])
            assert fit.log_r[g] == (D.RHO_MAX if f64["status"] == D.AT_UPPER else D.RHO_MIN) and np.isnan(fit.log_r_std[g])
            assert fit.dispersion[g] == 1.0 / float(bound_r32(f64["status"])) and fit.iterations[g] == 0
        assert fit.iterations[g] <= f32["iterations"] + 2
    print(f"{name}: worst rho {worst['rho']:.3g} se (bar {bars['rho']:.3g}), log_r_std {worst['std']:.3g} (bar {bars['std']:.3g}), "
          f"iterations {fit.iterations.max()}")
    assert worst["rho"] <= bars["rho"] and worst["std"] <= bars["std"]


@pytest.mark.parametrize("Nc,Ng,H", D.SHAPES)
def test_shapes(Nc, Ng, H):
    name = f"shape_{Nc}_{Ng}_{H}"
    fit = run(name)
    assert all(getattr(fit, f.name).shape == (Ng,) for f in fields(fit))
    assert_within_bars(name, fit)


def test_evaluate_only():
    """loglik and score at five r on the (257, 5, 1) problem; r = 1e6 is the cancellation case (the sum is 1e-7 of its parts)."""
    p = D.cases()[D.EVALUATE_CASE]
    bars, worst = D.bars(), dict(loglik=0.0, score=0.0)
    for r in D.EVALUATE_AT:
        fit = run(D.EVALUATE_CASE, start=1.0 / r, evaluate_only=True)
        r32 = np.float32(1.0 / (1.0 / r))
        for g in range(p["S"].shape[1]):
            ref, f32 = D.evaluated()[(r, g)]
            const = float(-gammaln(np.trunc(p["S"][:, g]) + 1).sum())
            d = D.point_distances(fit.loglik[g] - const, fit.score[g], ref)
            print(f"r = {r:g} gene {g}: loglik {d['loglik']:.3g} (restatement {D.point_distances(f32['L'], f32['fp'], ref)['loglik']:.3g}), "
                  f"score {d['score']:.3g} noise units (restatement {D.point_distances(f32['L'], f32['fp'], ref)['score']:.3g})")
            worst = {key: max(worst[key], d[key]) for key in worst}
            assert fit.status[g] == D.EVALUATED and fit.iterations[g] == 0 and fit.dispersion[g] == 1.0 / float(r32)
            assert fit.log_r[g] == math.log(float(r32)) or abs(fit.log_r[g] - math.log(float(r32))) <= 4 * D.EPS64 * abs(fit.log_r[g])
            if r in (0.05, 2.0):                                  # away from the bounds the curvature is no cancelled sum
                assert abs(fit.log_r_std[g] * math.sqrt(-ref["fpp"]) - 1) <= 1e-4
    print(f"evaluate-only: worst loglik {worst['loglik']:.3g} (bar {bars['loglik']:.3g}), score {worst['score']:.3g} (bar {bars['score']:.3g})")
    assert worst["loglik"] <= bars["loglik"] and worst["score"] <= bars["score"]


@pytest.mark.parametrize("name", ["large_u16", "large_f32"])
def test_large_counts(name):
    """Counts to 2.2e4 (7e4 in float32 storage), far above the histogram: the Stirling remainders carry most of the gamma terms."""
    assert D.cases()[name]["S"].max() > (65535 if name == "large_f32" else 2e4)
    fit = run(name)
    assert_within_bars(name, fit)
    assert abs(fit.log_r[0] + 2.788) < 2e-3


def test_bound_cases():
    for name, want in D.BOUND_CASES.items():
        fit = run(name)
        assert fit.status[0] == want, (name, fit.status[0])
        assert_within_bars(name, fit)
    fit = run("bound_binomial_prior")                         # the Gamma prior pulls the AT_UPPER gene inside
    assert fit.status[0] == D.CONVERGED and D.RHO_MIN < fit.log_r[0] < D.RHO_MAX
    assert_within_bars("bound_binomial_prior", fit)
    # a gene whose coefficients are not finite: NO_DATA, and its neighbours untouched
    p = D.cases()["shape_257_5_1"]
    nu = p["nu"].copy()
    nu[2, 0] = np.inf
    got = gene_dispersion(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], nu.T)
    ref = run("shape_257_5_1")
    assert got.status[2] == D.NO_DATA and np.isnan(got.log_r[2]) and np.isnan(got.dispersion[2]) and np.isnan(got.loglik[2])
    keep = [0, 1, 3, 4]
    assert all(np.array_equal(getattr(got, f.name)[keep], getattr(ref, f.name)[keep]) for f in fields(ref))


def joint_inputs(genes=slice(None)):
    p = D.joint_problem()
    return p["S"][:, genes].astype(np.float32), G.directions(p["phis"]), p["n"]


@lru_cache(maxsize=None)
def joint_fit():
    return gene_harmonics(*joint_inputs(), 1, 1, "NegativeBinomial", "mle")


def test_joint_fit():
    p, fit, bars = D.joint_problem(), joint_fit(), D.bars()
    B, logm = G.basis64(p["phis"], 1), np.log(p["n"])
    worst = dict(stat_r=0.0, stat_nu=0.0, z=0.0, rho=0.0)
    for g, (f64, f32) in enumerate(D.joint_solved()):
        r = float(np.float32(1.0 / fit.dispersion[g]))
        assert fit.dispersion[g] == 1.0 / r                       # the dispersion reported is that of the float32 r the fit was made at
        sr, dn = D.stationarity(fit.means[:, g], r, p["S"][:, g], B, logm)
        worst["stat_nu"] = max(worst["stat_nu"], dn)
        if g == D.POISSON_GENE:
            assert fit.dispersion_status[g] == D.AT_UPPER and np.isnan(fit.log_r_std[g]) and r == float(bound_r32(D.AT_UPPER))
            assert fit.overdispersion_p[g] == 1.0
            continue
        assert fit.dispersion_status[g] in D.INTERIOR, (g, fit.dispersion_status[g])
        worst["stat_r"] = max(worst["stat_r"], sr)
        worst["z"] = max(worst["z"], abs(math.log(r) - math.log(p["r_true"][g])) / fit.log_r_std[g])
        worst["rho"] = max(worst["rho"], abs(math.log(r) - f64["rho"]) * math.sqrt(f64["disp"]["info"]))
        assert abs(fit.log_r_std[g] / f64["disp"]["std"] - 1) <= 1e-4
        if p["r_true"][g] < 3:
            assert fit.overdispersion_p[g] < 1e-6, (g, fit.overdispersion_p[g])
        assert fit.overdispersion_p[g] == D.overdispersion_p(fit.overdispersion_lr[g])
        assert abs(fit.loglik[g] - G.logp64(p["S"][:, g], fit.means[:, g] @ B + logm, "NegativeBinomial", r).sum()) <= \
            G.bars()["loglik"] * G.EPS32 * f64["glm"]["abs"]
    print(f"joint fit: stationarity of rho {worst['stat_r']:.3g} se (bar {bars['stat_r']:.3g}), decrement of nu {worst['stat_nu']:.3g} "
          f"(bar {bars['stat_nu']:.3g}), rho from the reference {worst['rho']:.3g} se, from the truth {worst['z']:.3g} se, "
          f"rounds {fit.rounds.max()} (restatement {max(f32['rounds'] for _, f32 in D.joint_solved())})")
    assert worst["stat_r"] <= bars["stat_r"] and worst["stat_nu"] <= bars["stat_nu"]
    assert worst["z"] <= 4.0
    assert (fit.rounds >= 1).all() and (fit.rounds <= D.MAX_ROUNDS).all()
    assert (fit.status <= G.ROUNDING).all()


def test_null_model_has_its_own_dispersion():
    """lr_stat compares two maximised likelihoods: the null's is the reference's joint fit of the constant alone, and lies above the
    null fitted at the full model's dispersion."""
    p, fit = D.joint_problem(), joint_fit()
    B0, logm = G.basis64(p["phis"], 0), np.log(p["n"])
    at_full = gene_harmonics(*joint_inputs(), 1, 1, "NegativeBinomial", fit.dispersion)
    assert np.array_equal(at_full.means, fit.means) and np.array_equal(at_full.loglik, fit.loglik)     # the final fit is the one at the reported r
    gain = fit.loglik_null - at_full.loglik_null
    print("loglik_null gained by its own dispersion: min %.3g, max %.3g" % (gain.min(), gain.max()))
    assert (gain >= -G.bars()["lr"] * G.EPS32 * np.abs(fit.loglik_null)).all() and (gain > 0).sum() >= 35
    for g in (0, 7, 21):
        ref = D.joint64(p["S"][:, g], B0, logm)
        want = G.logp64(p["S"][:, g], ref["nu"] @ B0 + logm, "NegativeBinomial", math.exp(ref["rho"])).sum()
        assert abs(fit.loglik_null[g] - want) <= 1e-6 * abs(want) and fit.loglik_null[g] <= want + G.bars()["loglik"] * G.EPS32 * abs(want)
    assert np.array_equal(fit.lr_stat, 2.0 * (fit.loglik - fit.loglik_null))


def names(fit):
    return [f.name for f in fields(fit)] + (list(MLE_FIELDS) if isinstance(fit, GeneHarmonicFit) else [])


def same_bits(a, b):
    for name in names(a):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or (x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)), name


def test_bit_equal_across_chunks_storage_input_and_repetition():
    S, xy, n = joint_inputs(slice(20, 40))                        # 20 genes, the Poisson gene among them
    nb = dict(harmonics=1, noisemodel="NegativeBinomial", dispersion="mle")
    ref = gene_harmonics(S, xy, n, **nb)
    assert ref.dispersion_status[D.POISSON_GENE - 20] == D.AT_UPPER and len(set(ref.rounds)) > 1     # genes settle in different rounds
    for kw in (dict(chunk_genes=1), dict(chunk_genes=7), dict(chunk_genes=20), dict(storage="f32"), dict(storage="u16"), dict()):
        same_bits(ref, gene_harmonics(S, xy, n, **nb, **kw))
    same_bits(ref, gene_harmonics(sp.csr_matrix(S), xy, n, **nb, chunk_genes=7))
    full = joint_fit()
    assert all(getattr(ref, name) is not None for name in MLE_FIELDS)
    for name in names(ref):
        x = getattr(full, name)
        assert np.array_equal(getattr(ref, name), x[20:40] if x.shape[0] == 40 else x[..., 20:40], equal_nan=True), name
    # the dispersion kernel on its own
    p = D.cases()["shape_300_130_1"]
    args = (p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], p["nu"].T)
    one = gene_dispersion(*args)
    for kw in (dict(chunk_genes=1), dict(chunk_genes=7), dict(storage="f32"), dict()):
        same_bits(one, gene_dispersion(*args, **kw))
    same_bits(one, gene_dispersion(sp.csr_matrix(args[0]), *args[1:], chunk_genes=50))


def test_numeric_dispersion_gives_the_bits_it_gave():
    S, xy, n = joint_inputs(slice(0, 12))
    first = gene_harmonics(S, xy, n, 1, 1, "NegativeBinomial", 0.3)
    gene_harmonics(S, xy, n, 1, 1, "NegativeBinomial", "mle")
    second = gene_harmonics(S, xy, n, 1, 1, "NegativeBinomial", 0.3)
    same_bits(first, second)
    assert first.dispersion is None and first.overdispersion_p is None and first.rounds is None
    # and they are the bits of the kernel called the way the wrapper always called it: per-gene values of the same dispersion
    same_bits(first, gene_harmonics(S, xy, n, 1, 1, "NegativeBinomial", np.full(12, 0.3), rho_tol=1e-3))


def test_the_loop_through_the_containers():
    p = D.joint_problem()
    S = p["S"][:500, :12].astype(np.float32)
    obs = pd.DataFrame({"n_scounts": p["n"][:500]}, index=[f"c{i}" for i in range(500)])
    ad = AnnDataLite(S, S, obs=obs)
    ph = Phases.from_array(G.directions(p["phis"][:500]), cell_names=list(obs.index))
    cyc, fit = Cycle.from_phases_mle(ph, ad, 1, 1, "NegativeBinomial", "mle", return_fit=True)
    assert cyc.disp_pyro is not None and cyc.disp_pyro.shape == (12,) and np.array_equal(cyc.disp_pyro, fit.dispersion)
    assert (cyc.disp_pyro > 0).all() and np.isfinite(cyc.disp_pyro).all()
    out = Phases.from_array(G.directions(np.zeros(500)), cell_names=list(obs.index))
    best, prof = out.from_cycle_mle(cyc, ad, noisemodel="NegativeBinomial", dispersion=cyc.disp_pyro, return_profile=True)
    assert best.shape == (500,) and out.phi_xy.shape == (2, 500) and np.isfinite(out.phi_xy.values).all()
    got = np.arctan2(out.phi_xy.values[1], out.phi_xy.values[0])
    err = np.angle(np.exp(1j * (got - p["phis"][:500])))
    print("the loop: median |phase error| %.3g rad" % np.median(np.abs(err)))
    assert int(best.min()) >= 0 and int(best.max()) < 100 and bool(torch.isfinite(prof).all())


def test_refusals_through_the_c_abi():
    """Each with VC_ERR_ARG and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS:
        assert lib.vc_gene_dispersion(*disp_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="Poisson model has no dispersion"):
        gene_harmonics(np.ones((4, 2), np.float32), G.directions(np.arange(4.0)), np.ones(4), dispersion="mle")
