"""GPU: Cycle.from_phases_mle / velocycle_amd.gene_harmonics on the HIP kernel vc_gene_glm, judged by the float64 checker
(tests/gene_glm_checker.py) with bars that are 4 x its float32 restatement's own distance from float64 over these very problems
(tests/test_gene_harmonics_cpu.py asserts their cap and that every float64 fit converges)."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_glm_checker as G
from tests.test_gene_harmonics_cpu import glm_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.gene_harmonics import gene_harmonics

pytestmark = pytest.mark.gpu
DONE = (G.CONVERGED, G.ROUNDING)


def run(p, **kw):
    prior = p["prior"] if p["prior"] is not None else (None, None)
    return gene_harmonics(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], harmonics=p["H"], a=p["a"], noisemodel=p["noisemodel"],
                          dispersion=p["dispersion"] if p["dispersion"] is not None else 0.3, prior_means=prior[0], prior_stds=prior[1], **kw)


@lru_cache(maxsize=None)
def fitted(name):
    return run(G.cases()[name])


def same_bits(a, b, genes=slice(None), other=slice(None)):
    """Every array of two fits, bit for bit (NaN == NaN), on the given genes of each."""
    for f in fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        x, y = (x[:, genes], y[:, other]) if f.name in ("means", "stds") else (x[genes], y[other])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f.name


def assert_within_bars(name, fit, solved=None, max_iter_over=2, genes=None):
    """Status, iterations and the four yardsticks of every gene against the float64 fits of the case."""
    solved = G.solved(name) if solved is None else solved
    bars = G.bars()
    worst = dict(coef=0.0, std=0.0, loglik=0.0, lr=0.0)
    for g, (f64, n64, f32, n32) in enumerate(solved):
        if genes is not None and g not in genes:
            continue
        assert fit.status[g] in DONE, (name, g, fit.status[g])
        assert fit.iterations[g] <= f32["iterations"] + max_iter_over, (name, g, fit.iterations[g], f32["iterations"])
        d = G.distances(fit.means[:, g], fit.stds[:, g], fit.loglik[g], fit.lr_stat[g], f64, n64)
        for key in worst:
            worst[key] = max(worst[key], d[key])
    print(f"{name}: worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()) +
          f"; iterations <= {int(fit.iterations.max())}; ROUNDING stops {int((fit.status == G.ROUNDING).sum())}")
    for key in worst:
        assert worst[key] <= bars[key], (name, key, worst[key], bars[key])


@pytest.mark.parametrize("noise,disp", G.NOISES)
@pytest.mark.parametrize("Nc,Ng,H", G.SHAPES)
def test_shapes(Nc, Ng, H, noise, disp):
    name = f"shape_{Nc}_{Ng}_{H}_{noise}"
    fit = fitted(name)
    K = 2 * H + 1
    assert fit.means.shape == fit.stds.shape == (K, Ng) and fit.cov.shape == (Ng, K, K) and fit.dof == 2 * H
    assert np.array_equal(fit.stds, np.sqrt(np.einsum("gii->ig", fit.cov))) and np.array_equal(fit.cov, fit.cov.transpose(0, 2, 1))
    assert_within_bars(name, fit)
    assert (fit.lr_stat >= -G.bars()["lr"] * G.EPS32 * np.array([s[0]["abs"] for s in G.solved(name)])).all()
    assert ((fit.p_value >= 0) & (fit.p_value <= 1)).all()
    p = G.cases()[name]
    same_bits(fit, run(p))                                         # a second run
    same_bits(fit, run(p, storage="f32"))
    same_bits(fit, run(p, storage="u16"))
    for chunk in sorted({1, 7, Ng}):
        same_bits(fit, run(p, chunk_genes=chunk))


def test_per_gene_dispersion_and_csr_through_the_classmethod():
    name = "per_gene_dispersion"
    p = G.cases()[name]
    S = p["S"].astype(np.float32)
    obs = pd.DataFrame({"n_scounts": p["n"]}, index=[f"c{i}" for i in range(S.shape[0])])
    ph = Phases.from_array(10.0 * G.directions(p["phis"]), cell_names=list(obs.index))
    got = {}
    for kind, layer in (("dense", S), ("csr", sp.csr_matrix(S))):
        ad = AnnDataLite(layer, layer, obs=obs.copy())
        got[kind] = Cycle.from_phases_mle(ph, ad, p["H"], 1, "NegativeBinomial", p["dispersion"], return_fit=True)
    (cyc, fit), (cyc2, fit2) = got["dense"], got["csr"]
    same_bits(fit, fit2)
    assert cyc.means.equals(cyc2.means) and cyc.stds.equals(cyc2.stds)
    assert list(cyc.means.index) == list(cyc.stds.index) == ["nu0", "nu1_cos", "nu1_sin", "nu2_cos", "nu2_sin"]
    assert list(cyc.means.columns) == list(cyc.stds.columns) == list(ad.var.index)
    assert np.array_equal(cyc.means.values, fit.means) and np.array_equal(cyc.stds.values, np.sqrt(np.einsum("gii->ig", fit.cov)))
    assert_within_bars(name, fit)
    # the length of the phase directions carries nothing
    same_bits(fit, run(p))


@pytest.mark.parametrize("noise", [n for n, _ in G.NOISES])
def test_large_counts(noise):
    for kind, extra in (("u16", None), ("f32", 70000.0)):
        name = f"large_{kind}_{noise}"
        p = G.cases()[name]
        assert p["S"].max() >= 1e4
        fit = fitted(name)
        assert (fit.iterations <= 10).all(), fit.iterations
        assert_within_bars(name, fit)
        if p["S"].max() <= 65535:
            same_bits(fit, run(p, storage="u16"))
            same_bits(fit, run(p, storage="f32"))
        else:
            with pytest.raises(ValueError, match="u16"):
                run(p, storage="u16")


def test_separation():
    S, phis, n = G.separated()
    Ng = S.shape[1]
    p = G.problem(S, phis, n, 3, "Poisson")
    fit = run(p)
    assert fit.status[-1] in (G.UNBOUNDED, G.MAX_ITER), fit.status
    # finite or flagged: the flagged gene's own numbers are finite here too (the last point inside the bound and its curvature)
    assert np.isfinite(fit.means).all() and np.isfinite(fit.loglik).all() and np.isfinite(fit.loglik_null).all()
    assert set(fit.status[:-1]) <= set(DONE)
    # the neighbours do not know of it
    same_bits(fit, run(G.problem(S[:, :-1], phis, n, 3, "Poisson")), genes=slice(0, Ng - 1))
    # with a prior the gene has a posterior mode
    name = "separation_prior"
    fit = fitted(name)
    assert (fit.status == G.CONVERGED).all() and (fit.iterations <= 8).all(), (fit.status, fit.iterations)
    assert_within_bars(name, fit)


def test_prior():
    ml_name = "shape_257_5_1_NegativeBinomial"
    ml = fitted(ml_name)
    wide = fitted("prior_wide")
    assert_within_bars(ml_name, wide)                             # stds of 1e6: the maximum-likelihood fit, held to ITS float64 optimum
    assert np.abs(wide.means - ml.means).max() <= 1e-6
    p = G.cases()[ml_name]
    means = np.vstack([np.zeros((1, 5)), np.full((1, 5), 0.25), np.full((1, 5), -0.125)])
    stds = np.vstack([np.full((1, 5), 10.0), np.full((2, 5), 1e-3)])
    tight = run(G.problem(p["S"], p["phis"], p["n"], 1, "NegativeBinomial", 0.3, (means, stds)))
    assert set(tight.status) <= set(DONE)
    assert np.abs(tight.means[1:] - means[1:]).max() <= 1e-2
    assert (tight.stds[1:] <= 1e-3 * (1 + 1e-9)).all()
    # a coefficient without a finite prior mean has no prior
    nan_means, nan_stds = np.full((3, 5), np.nan), np.ones((3, 5))
    same_bits(ml, run(G.problem(p["S"], p["phis"], p["n"], 1, "NegativeBinomial", 0.3, (nan_means, nan_stds))))


def test_periodicity():
    name = "periodicity"
    fit = fitted(name)
    assert_within_bars(name, fit)
    solved = G.solved(name)
    lr64 = np.array([2 * (f["loglik"] - n["loglik"]) for (f, n, _, _) in solved])
    scale = G.bars()["lr"] * G.EPS32 * np.array([f["abs"] for (f, _, _, _) in solved])
    for i in range(len(lr64)):
        for j in range(len(lr64)):
            if lr64[i] - lr64[j] > scale[i] + scale[j]:
                assert fit.lr_stat[i] > fit.lr_stat[j], (i, j)
    assert int(np.argmax(fit.lr_stat)) == G.PERMUTED_GENE and fit.p_value[G.PERMUTED_GENE] < 1e-100
    shuffled = fitted("permuted")
    assert_within_bars("permuted", shuffled)
    assert shuffled.p_value[0] > 1e-3, shuffled.p_value


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    one = C.c_void_p(64)
    assert lib.vc_gene_glm(*glm_args(K=2)) == _lib.VC_ERR_ARG and b"K must be" in lib.vc_last_error(None)
    for name in ("nu", "cov", "ll", "dec", "it", "st"):
        assert lib.vc_gene_glm(*glm_args(**{name: None})) == _lib.VC_ERR_ARG and b"null output" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(noise=_lib.NOISE["Lognormal"])) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(pm=one)) == _lib.VC_ERR_ARG and b"prior" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(pp=one)) == _lib.VC_ERR_ARG and b"prior" in lib.vc_last_error(None)
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(NotImplementedError):
        gene_harmonics(np.ones((4, 2), np.float32), G.directions(np.arange(4.0)), np.ones(4), noisemodel="Lognormal")
