"""CPU: the checker of the per-gene harmonic regression (tests/gene_glm_checker.py) against what is known in closed form and against
the simulation's truth; the bars it sets for tests/test_hip_gene_harmonics.py; the public face of `velocycle_amd.gene_harmonics` and
`Cycle.from_phases_mle` (refusals before any device work, container plumbing); the C ABI declaration, its binding and its refusals."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gene_glm_checker as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_optimum_recovers_the_simulation():
    """simulate_counts draws mu = exp(nu . zeta) without a count factor: with n_c = N for every cell the model's nu_0 is the simulated
    one minus log N.  Negative binomial at the simulated dispersions: the model is the generating one."""
    sim = G.simulated(3000, 8)
    N = float(sim["S"].sum(1).mean())
    B = G.basis64(sim["phis"], 1)
    logm = np.full(3000, np.log(N))
    for g in range(8):
        fit = G.newton64(sim["S"][:, g], B, logm, "NegativeBinomial", 1.0 / sim["shape_inv"][g])
        assert fit["status"] == G.CONVERGED
        z = (fit["nu"] + np.array([np.log(N), 0, 0]) - sim["nu"][g]) / fit["std"]
        assert np.abs(z).max() <= 5.0, (g, z)


@pytest.mark.parametrize("noise,disp", G.NOISES)
def test_gradient_vanishes_at_the_float64_optimum(noise, disp):
    sim = G.simulated(3000, 8)
    B, logm = G.basis64(sim["phis"], 2), np.log(sim["n"])
    r = None if disp is None else 1.0 / disp
    for g in range(8):
        k = sim["S"][:, g]
        fit = G.newton64(k, B, logm, noise, r)
        mu = np.exp(fit["nu"] @ B + logm)
        res = k - mu if r is None else (k - mu) * r / (r + mu)
        assert (np.abs(B @ res) <= 1e-9 * (np.abs(B * res)).sum(1)).all()
        # and the Hessian the checker factors is the derivative of its gradient
        h = 1e-6
        for i in range(B.shape[0]):
            d = np.zeros(B.shape[0])
            d[i] = h
            num = (G.eval64(fit["nu"] + d, k, B, logm, noise, r)["grad"] - G.eval64(fit["nu"] - d, k, B, logm, noise, r)["grad"]) / (2 * h)
            assert np.allclose(-num, fit["hess"][i], rtol=1e-5, atol=1e-5 * np.abs(fit["hess"]).max())


def test_poisson_constant_model_is_the_closed_form():
    sim = G.simulated(257, 5)
    logm = 0.7 * np.log(sim["n"])
    for g in range(5):
        fit = G.newton64(sim["S"][:, g], G.basis64(sim["phis"], 0), logm, "Poisson")
        want = np.log(sim["S"][:, g].sum() / (sim["n"] ** 0.7).sum())
        assert fit["status"] == G.CONVERGED and abs(fit["nu"][0] - want) <= 1e-13 * max(1.0, abs(want))
        assert abs(fit["std"][0] - 1 / np.sqrt(sim["S"][:, g].sum())) <= 1e-12


def test_every_float64_fit_of_the_gpu_cases_converges():
    for name in G.cases():
        for (f64, n64, f32, n32) in G.solved(name):
            assert f64["status"] == G.CONVERGED and n64["status"] == G.CONVERGED, name
            assert f32["status"] in (G.CONVERGED, G.ROUNDING) and n32["status"] in (G.CONVERGED, G.ROUNDING), name
            assert np.isfinite(f64["std"]).all()


def test_bars_come_from_the_restatement():
    bars = G.bars()
    print("bars (4 x the float32 restatement's worst over the GPU cases):", {k: float(f"{v:.4g}") for k, v in bars.items()})
    assert 0 < bars["coef"] <= G.COEF_CAP
    assert 0 < bars["std"] < 1e-3 and 0 < bars["loglik"] and 0 < bars["lr"]
    worst_iter = max(f32["iterations"] for name in G.cases() for (_, _, f32, _) in G.solved(name))
    assert worst_iter <= 8


def test_rounding_rule_ends_what_the_decrement_cannot():
    """Below the float32 floor of the gradient the decrement stops falling: with a tol under that floor (here 0) only the ROUNDING rule
    ends the iteration, within a few steps and within the coefficient bar; without it the restatement spends max_iter."""
    for name in ("large_u16_Poisson", "large_f32_NegativeBinomial", "shape_257_5_1_Poisson"):
        p = G.cases()[name]
        k, B, logm, r, prior = G._gene_inputs(p, 0)
        f64 = G.solved(name)[0][0]
        with_rule = G.restate32(k, B, logm, p["noisemodel"], r, tol=0.0)
        without = G.restate32(k, B, logm, p["noisemodel"], r, tol=0.0, rounding_rule=False)
        d = with_rule["nu"] - f64["nu"]
        assert with_rule["status"] == G.ROUNDING and with_rule["iterations"] <= 10 and np.sqrt(d @ f64["hess"] @ d) <= G.bars()["coef"], name
        assert without["status"] == G.MAX_ITER and without["iterations"] == 25, name


def test_separated_gene_has_no_float64_optimum_without_a_prior():
    S, phis, n = G.separated()
    fit = G.newton64(S[:, -1], G.basis64(phis, 3), np.log(n), "Poisson")
    assert fit["status"] != G.CONVERGED


def test_permuted_phases_are_not_called_periodic():
    (f64, n64, _, _), = G.solved("permuted")
    assert G.chi2_sf_even(2 * (f64["loglik"] - n64["loglik"]), 2) > 1e-3
    lr = [2 * (f["loglik"] - n["loglik"]) for (f, n, _, _) in G.solved("periodicity")]
    assert int(np.argmax(lr)) == G.PERMUTED_GENE and G.chi2_sf_even(max(lr), 2) < 1e-100


def test_p_value_is_the_chi_square_survival_function():
    from scipy.stats import chi2
    from velocycle_amd.gene_harmonics import GeneHarmonicFit
    x = np.array([0.0, 0.3, 2.0, 17.5, 140.0, np.nan])
    for H in (1, 2, 3):
        K = 2 * H + 1
        fit = GeneHarmonicFit(means=np.zeros((K, 6)), stds=np.ones((K, 6)), cov=np.zeros((6, K, K)), loglik=x / 2, loglik_null=np.zeros(6),
                              decrement=np.zeros(6), iterations=np.zeros(6, np.int32), status=np.zeros(6, np.int32))
        assert fit.dof == 2 * H and np.allclose(fit.lr_stat[:5], x[:5])
        assert np.allclose(fit.p_value[:5], chi2.sf(x[:5], 2 * H), rtol=1e-12, atol=0) and np.isnan(fit.p_value[5])
        assert np.allclose([G.chi2_sf_even(v, 2 * H) for v in x[:5]], chi2.sf(x[:5], 2 * H), rtol=1e-12, atol=0)
    fit0 = GeneHarmonicFit(means=np.zeros((1, 2)), stds=np.ones((1, 2)), cov=np.zeros((2, 1, 1)), loglik=np.zeros(2), loglik_null=np.zeros(2),
                           decrement=np.zeros(2), iterations=np.zeros(2, np.int32), status=np.zeros(2, np.int32))
    assert fit0.dof == 0 and (fit0.p_value == 1).all()


def test_basis_from_directions_is_the_fourier_basis():
    from velocycle_amd.gene_harmonics import fourier_basis_from_directions
    phis = G.simulated(257, 5)["phis"]
    got = fourier_basis_from_directions(7.5 * G.directions(phis), 3).numpy()
    assert got.shape == (7, 257) and np.abs(got - G.basis64(phis, 3)).max() <= 1e-14


def test_signature():
    from velocycle_amd.containers import Cycle
    from velocycle_amd.gene_harmonics import gene_harmonics
    sig = inspect.signature(Cycle.from_phases_mle)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos == [("phases", inspect.Parameter.empty), ("data", inspect.Parameter.empty), ("harmonics", 1), ("a", 1),
                   ("noisemodel", "Poisson"), ("dispersion", 0.3)]
    assert {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == {"layer": "spliced", "prior": None, "return_fit": False}
    sig = inspect.signature(gene_harmonics)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos == [("counts", inspect.Parameter.empty), ("directions", inspect.Parameter.empty), ("n_scounts", inspect.Parameter.empty),
                   ("harmonics", 1), ("a", 1), ("noisemodel", "Poisson"), ("dispersion", 0.3)]
    assert {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == \
        {"prior_means": None, "prior_stds": None, "tol": 1e-10, "max_iter": 25, "device": None, "chunk_genes": None, "storage": "auto"}


def _objects(Nc=6, Ng=4):
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import Phases
    S = (np.arange(Nc * Ng, dtype=np.float32).reshape(Nc, Ng) % 5) + 1
    ad = AnnDataLite(S, S, obs=pd.DataFrame({"n_scounts": S.sum(1)}, index=[f"c{i}" for i in range(Nc)]))
    ph = Phases.from_array(G.directions(np.linspace(0.1, 6.0, Nc)) * 3.0, cell_names=list(ad.obs.index))
    return ad, ph


@pytest.fixture
def no_device(monkeypatch):
    from velocycle_amd import _lib

    def reached(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(_lib, "load", reached)
    monkeypatch.setattr(torch.cuda, "is_available", reached)


def test_refusals_fire_before_the_device(no_device):
    import scipy.sparse as sp
    from velocycle_amd.containers import Cycle
    from velocycle_amd.gene_harmonics import gene_harmonics
    S = (np.arange(24, dtype=np.float32).reshape(6, 4) % 5) + 1
    xy, n = G.directions(np.linspace(0.1, 6.0, 6)), S.sum(1)
    with pytest.raises(NotImplementedError, match="Not implemented yet, sorry"):
        gene_harmonics(S, xy, n, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="harmonics"):
        gene_harmonics(S, xy, n, harmonics=4)
    with pytest.raises(ValueError, match="harmonics"):
        gene_harmonics(S, xy, n, harmonics=-1)
    with pytest.raises(ValueError, match="directions"):
        gene_harmonics(S, xy[:, :5], n)
    with pytest.raises(ValueError, match="directions"):
        gene_harmonics(S, xy.T, n)
    bad = xy.copy()
    bad[:, 2] = 0.0
    with pytest.raises(ValueError, match="non-zero length"):
        gene_harmonics(S, bad, n)
    with pytest.raises(ValueError, match="n_scounts"):
        gene_harmonics(S, xy, n[:5])
    with pytest.raises(ValueError, match="n_scounts"):
        gene_harmonics(S, xy, np.where(np.arange(6) == 3, 0.0, n))
    with pytest.raises(ValueError, match="dispersion"):
        gene_harmonics(S, xy, n, noisemodel="NegativeBinomial", dispersion=0.0)
    with pytest.raises(ValueError, match="dispersion"):
        gene_harmonics(S, xy, n, noisemodel="NegativeBinomial", dispersion=np.array([0.3, 0.3, -1.0, 0.3]))
    with pytest.raises(ValueError, match="dispersion"):
        gene_harmonics(S, xy, n, noisemodel="NegativeBinomial", dispersion=np.array([0.3, 0.3]))
    with pytest.raises(ValueError, match="both"):
        gene_harmonics(S, xy, n, prior_means=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="prior"):
        gene_harmonics(S, xy, n, prior_means=np.zeros((5, 4)), prior_stds=np.ones((5, 4)))
    with pytest.raises(ValueError, match="prior_stds"):
        gene_harmonics(S, xy, n, prior_means=np.zeros((3, 4)), prior_stds=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="tol"):
        gene_harmonics(S, xy, n, tol=-1.0)
    with pytest.raises(ValueError, match="max_iter"):
        gene_harmonics(S, xy, n, max_iter=0)
    # genes without a count: how many, and what to do with them -- dense, sparse, and counts that truncate to zero
    Z = S.copy()
    Z[:, 1] = 0
    Z[:, 3] = 0.5
    for counts in (Z, sp.csr_matrix(Z), torch.tensor(Z)):
        with pytest.raises(ValueError, match=r"2 of 4 genes have no count.*filter"):
            gene_harmonics(counts, xy, n)
    # the classmethod refuses the same, and what only it can see
    ad, ph = _objects()
    with pytest.raises(NotImplementedError):
        Cycle.from_phases_mle(ph, ad, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="layer"):
        Cycle.from_phases_mle(ph, ad, layer="nope")
    with pytest.raises(ValueError, match="cells"):
        Cycle.from_phases_mle(type(ph).from_array(ph.phi_xy.values[:, :5], cell_names=list(ad.obs.index)[:5]), ad)
    other = type(ph).from_array(ph.phi_xy.values, cell_names=[f"x{i}" for i in range(6)])
    with pytest.raises(ValueError, match="cells"):
        Cycle.from_phases_mle(other, ad)
    with pytest.raises(ValueError, match="genes"):
        Cycle.from_phases_mle(ph, ad, prior=Cycle.trivial_prior(["a", "b", "c", "d"], harmonics=1))
    with pytest.raises(ValueError, match="harmonics"):
        Cycle.from_phases_mle(ph, ad, prior=Cycle.trivial_prior(list(ad.var.index), harmonics=2))
    ad.obs.loc[ad.obs.index[2], "n_scounts"] = 0.0
    with pytest.raises(ValueError, match="n_scounts"):
        Cycle.from_phases_mle(ph, ad)


def test_container_plumbing(monkeypatch):
    from velocycle_amd import gene_harmonics as GH
    from velocycle_amd.containers import Cycle
    ad, ph = _objects()
    seen = {}

    def fake(counts, directions, n_scounts, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, **kw):
        seen.update(counts=counts, directions=directions, n_scounts=n_scounts, harmonics=harmonics, a=a, noisemodel=noisemodel,
                    dispersion=dispersion, kw=kw)
        K, Ng = 2 * harmonics + 1, counts.shape[1]
        means = np.arange(K * Ng, dtype=np.float64).reshape(K, Ng)
        return GH.GeneHarmonicFit(means=means, stds=means + 1, cov=np.zeros((Ng, K, K)), loglik=np.ones(Ng), loglik_null=np.zeros(Ng),
                                  decrement=np.zeros(Ng), iterations=np.zeros(Ng, np.int32), status=np.zeros(Ng, np.int32))
    monkeypatch.setattr(GH, "gene_harmonics", fake)
    prior = Cycle.trivial_prior(list(ad.var.index), harmonics=2)
    cyc, fit = Cycle.from_phases_mle(ph, ad, 2, 0.5, "NegativeBinomial", np.full(4, 0.2), prior=prior, return_fit=True, chunk_genes=3, tol=1e-8)
    assert isinstance(cyc, Cycle) and list(cyc.means.columns) == list(ad.var.index) and list(cyc.stds.columns) == list(ad.var.index)
    assert list(cyc.means.index) == list(Cycle.from_array(np.zeros((5, 4)), np.ones((5, 4))).means.index) == \
        ["nu0", "nu1_cos", "nu1_sin", "nu2_cos", "nu2_sin"]
    assert (cyc.means.values == fit.means).all() and (cyc.stds.values == fit.stds).all() and cyc.harmonics == 2
    assert seen["harmonics"] == 2 and seen["a"] == 0.5 and seen["noisemodel"] == "NegativeBinomial" and (seen["dispersion"] == 0.2).all()
    assert seen["directions"].shape == (2, 6) and (seen["directions"] == ph.phi_xy.values).all()
    assert (np.asarray(seen["n_scounts"]) == ad.obs.n_scounts.values).all()
    assert seen["kw"]["chunk_genes"] == 3 and seen["kw"]["tol"] == 1e-8
    assert (seen["kw"]["prior_means"] == prior.means.values).all() and (seen["kw"]["prior_stds"] == prior.stds.values).all()
    assert (np.asarray(seen["counts"]) == np.asarray(ad.layers["spliced"])).all()
    only = Cycle.from_phases_mle(ph, ad)
    assert isinstance(only, Cycle) and only.harmonics == 1 and seen["kw"]["prior_means"] is None
    # what it returns is what preprocess_for_* and condition_on consume: a Cycle like any other
    assert only.means_tensor.shape == (3, 4) and only[list(ad.var.index)[:2]].shape == (3, 2)


def test_header_declares_and_lib_binds_vc_gene_glm():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert re.search(r"\bint vc_gene_glm\(const void\* counts_dev, int count_kind", hdr)
    assert " *   vc_gene_glm " in hdr and "#define VC_ABI_VERSION 2" in hdr
    for i, name in enumerate(["CONVERGED", "ROUNDING", "UNBOUNDED", "SINGULAR", "MAX_ITER"]):
        assert f"#define VC_GLM_{name} {i}" in hdr and getattr(_lib, f"VC_GLM_{name}") == i == getattr(G, name)
    decl = re.search(r"\bint vc_gene_glm\(([^;]*)\);", hdr).group(1)
    assert "vc_gene_glm" in _lib.EXPORTS and len(_lib.EXPORTS["vc_gene_glm"][1]) == len(decl.split(",")) == 21
    assert decl.rstrip().endswith("void* hip_stream")


def glm_args(**k):
    """Arguments of vc_gene_glm with pointers that are never dereferenced: every call made with them is refused before the launch."""
    one = C.c_void_p(64)
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("noise", 1), k.get("r", None), k.get("pm", None), k.get("pp", None), k.get("tol", 1e-10),
            k.get("max_iter", 25), k.get("nu", one), k.get("cov", one), k.get("ll", one), k.get("dec", one), k.get("it", one),
            k.get("st", one), None]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)
    assert lib.vc_gene_glm(*glm_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    for K in (0, 2, 4, 9):
        assert lib.vc_gene_glm(*glm_args(K=K)) == _lib.VC_ERR_ARG and b"K must be" in lib.vc_last_error(None)
    for name in ("counts", "basis", "logm", "nu", "cov", "ll", "dec", "it", "st"):
        assert lib.vc_gene_glm(*glm_args(**{name: None})) == _lib.VC_ERR_ARG and b"null" in lib.vc_last_error(None), name
    assert lib.vc_gene_glm(*glm_args(Nc=0)) == _lib.VC_ERR_ARG
    assert lib.vc_gene_glm(*glm_args(Ng=0)) == _lib.VC_ERR_ARG
    assert lib.vc_gene_glm(*glm_args(stride=3)) == _lib.VC_ERR_ARG and b"gene_stride" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(max_iter=0)) == _lib.VC_ERR_ARG and b"max_iter" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(tol=-1e-3)) == _lib.VC_ERR_ARG and b"tol" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(tol=float("nan"))) == _lib.VC_ERR_ARG
    assert lib.vc_gene_glm(*glm_args(pm=one)) == _lib.VC_ERR_ARG and b"prior" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(pp=one)) == _lib.VC_ERR_ARG and b"prior" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(kind=7)) == _lib.VC_ERR_ARG
    assert lib.vc_gene_glm(*glm_args(noise=0)) == _lib.VC_ERR_ARG and b"r_dev" in lib.vc_last_error(None)
    assert lib.vc_gene_glm(*glm_args(noise=5)) == _lib.VC_ERR_ARG


def test_default_chunk_stays_under_the_stated_bound():
    from velocycle_amd import gene_harmonics as GH
    from velocycle_amd import phase_mle
    for Nc in (1, 257, 50000, 10 ** 8):
        n = GH.default_chunk_genes(Nc)
        assert n >= 1 and (n == 1 or 4 * Nc * n <= phase_mle.CHUNK_BYTES)
