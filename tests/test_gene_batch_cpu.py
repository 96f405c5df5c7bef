"""CPU: the checker of the batch-aware harmonic regression (tests/gene_batch_checker.py) against itself and against finite differences;
the bars it sets for tests/test_hip_gene_batch.py; every refusal of `velocycle_amd.gene_batch`, `Cycle.from_phases_batch_mle` and
`Phases.from_cycle_batch_mle` that needs no device; the new signatures; the container plumbing; the C ABI declaration and its refusals."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gene_batch_checker as BC
from tests import gene_glm_checker as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONE = (G.CONVERGED, G.ROUNDING)


def test_every_fit_of_the_gpu_cases_ends_at_its_optimum():
    """No case is left out of a comparison: the float64 reference converges and the restatement ends CONVERGED or ROUNDING, everywhere."""
    for name in BC.cases():
        for (f64, n64, f32, n32) in BC.solved(name):
            assert f64["status"] == G.CONVERGED and n64["status"] == G.CONVERGED, name
            assert f32["status"] in DONE and n32["status"] in DONE, name
            assert np.isfinite(f64["std"]).all() and np.isfinite(f32["std"]).all(), name


def test_bars_come_from_the_restatement():
    bars = BC.bars()
    print("bars (4 x the float32 restatement's worst over the GPU cases):", {k: float(f"{v:.4g}") for k, v in bars.items()})
    assert 0 < bars["coef"] <= BC.COEF_CAP
    assert 0 < bars["std"] < 1e-3 and 0 < bars["dstd"] < 1e-3 and 0 < bars["loglik"] and 0 < bars["lr"]
    # dense reference against restatement within the bars, case by case (the bars are 4 x the worst of exactly these distances)
    for name in BC.cases():
        for (f64, n64, f32, n32) in BC.solved(name):
            K = f64["K"]
            d = BC.distances(f32["nu"][:K], f32["nu"][K:], f32["std"][:K], f32["std"][K:], f32["loglik"],
                             2 * (f32["loglik"] - n32["loglik"]), f64, n64)
            assert all(d[key] <= bars[key] for key in BC.YARDSTICKS), (name, d)
    assert max(f32["iterations"] for name in BC.cases() for (_, _, f32, _) in BC.solved(name)) <= 8


def _system(name, g, at=None):
    """The dense penalised system of gene g of a case as a function of the point, a point (default: the start), K and the prior."""
    p = BC.cases()[name]
    k, B, lab, logm, r, prior, dprior = BC.gene_inputs(p, g)
    Ba, pa = BC.augmented(B, lab, prior, dprior)
    pm, pp = G._prior(pa, Ba.shape[0])
    x = G.start(k, logm, Ba.shape[0], pm, pp) if at is None else at
    return (lambda y: G.eval64(y, k, Ba, logm, p["noisemodel"], r, pm, pp)), x, B.shape[0], pm, pp


@pytest.mark.parametrize("name", ["seven_1_NegativeBinomial", "seven_2_Poisson", "max_batches", "nu_prior", "large_u16_NegativeBinomial"])
def test_schur_step_is_the_dense_step(name):
    """Two backward-stable solutions of one system differ by a small multiple of eps64 cond(H): about 1e-12 relative at cond 1e3..1e4 ..."""
    eps64 = float(np.finfo(np.float64).eps)
    for g in range(2):
        ev, x, K, pm, pp = _system(name, g)
        for _ in range(3):                                           # at the start and at the next two Newton points
            e = ev(x)
            Hm, gr = e["hess"], e["grad"]                            # penalised
            dense = np.linalg.solve(Hm, gr)
            d = x - pm
            got, dec, S, D, h = BC.schur(gr + pp * d, Hm - np.diag(pp), K, pp[:K], d[:K], pp[K:], d[K:])
            # ... and the Schur form is handed the unpenalised gradient, formed here as gr + pp d: its rounding, through H^-1
            inv = np.linalg.inv(Hm)
            fed = 8 * eps64 * (np.abs(gr) + np.abs(pp * d))
            bar = 8 * eps64 * np.linalg.cond(Hm)
            dist = np.abs(got - dense).max()
            print(f"{name} gene {g}: step distance {dist / np.abs(dense).max():.2e} (bar {bar:.2e})")
            assert dist <= bar * np.abs(dense).max() + (np.abs(inv) @ fed).max(), (name, g)
            assert abs(dec - gr @ dense) <= bar * abs(gr @ dense) + 2 * np.abs(dense) @ fed
            # the blocks of the inverse the kernel reports
            Sinv = np.linalg.inv(S)
            assert np.abs(Sinv - inv[:K, :K]).max() <= bar * np.abs(inv[:K, :K]).max()
            assert np.allclose(1 / D + np.einsum("bi,ij,bj->b", h, Sinv, h) / D ** 2, np.diag(inv)[K:], rtol=bar, atol=0)
            x = x + dense


@pytest.mark.parametrize("name", ["seven_1_NegativeBinomial", "seven_2_Poisson", "silent_batch"])
def test_hessian_is_the_derivative_of_the_gradient(name):
    f64 = BC.solved(name)[0][0]
    ev, x, K, _, _ = _system(name, 0, at=f64["nu"])
    hess = ev(x)["hess"]
    hstep = 1e-6
    for i in range(x.size):
        d = np.zeros(x.size)
        d[i] = hstep
        num = (ev(x + d)["grad"] - ev(x - d)["grad"]) / (2 * hstep)
        assert np.allclose(-num, hess[i], rtol=1e-5, atol=1e-5 * np.abs(hess).max()), (name, i)
    assert np.abs(ev(x)["grad"]).max() <= 1e-8 * np.abs(hess).max()


def test_a_silent_batch_has_a_finite_offset_under_the_prior():
    f64, _, f32, _ = BC.solved("silent_batch")[0]
    assert f64["status"] == G.CONVERGED and f32["status"] in DONE
    K = f64["K"]
    assert -50 < f64["nu"][K + 1] < f64["nu"][K] and -50 < f64["nu"][K + 1] < f64["nu"][K + 2]


def test_round_trip_seed_shows_the_bias_the_feature_removes():
    """The single-sample fit of the round trip's data puts a true sin / cos coefficient outside 4 of its own standard errors; the
    batch-aware float64 fit covers every simulated offset within 4 of its standard errors."""
    sim = BC.round_trip()
    assert BC.single_sample_bias(sim) > 4.0
    B, logm = G.basis64(sim["phis"], 1), np.log(sim["n"])
    for g in range(sim["S"].shape[1]):
        fit = BC.newton64(sim["S"][:, g], B, sim["labels"], logm, "NegativeBinomial", 1 / 0.3)
        assert fit["status"] == G.CONVERGED
        z = (fit["nu"][3:] - sim["dnu"][:, g]) / fit["std"][3:]
        assert np.abs(z).max() <= 4.0 * (1 - 1e-3), (g, z)              # with room for the device's distance from this fit


def test_signatures():
    from velocycle_amd.containers import Cycle, Phases
    from velocycle_amd.gene_batch import GeneBatchHarmonicFit, gene_harmonics_batched
    E = inspect.Parameter.empty

    def split(f):
        sig = inspect.signature(f)
        return ([(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD],
                {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY})
    pos, kw = split(gene_harmonics_batched)
    assert pos == [("counts", E), ("directions", E), ("n_scounts", E), ("batches", E), ("harmonics", 1), ("a", 1), ("noisemodel", "Poisson"),
                   ("dispersion", 0.3)]
    assert kw == {"delta_nu_prior": (0.0, 0.5), "prior_means": None, "prior_stds": None, "tol": 1e-10, "max_iter": 25, "device": None,
                  "chunk_genes": None, "storage": "auto"}
    pos, kw = split(Cycle.from_phases_batch_mle)
    assert pos == [("phases", E), ("data", E), ("batch_design", E), ("harmonics", 1), ("a", 1), ("noisemodel", "Poisson"), ("dispersion", 0.3)]
    assert kw == {"layer": "spliced", "delta_nu_prior": (0.0, 0.5), "prior": None, "return_fit": False}
    pos, kw = split(Phases.from_cycle_batch_mle)
    assert pos == [("self", E), ("cycle", E), ("data", E), ("batch_design", E), ("delta_nu", E), ("a", 1), ("bins", 100), ("concentration", 10.),
                   ("noisemodel", "Poisson"), ("dispersion", 0.3)]
    assert kw == {"device": None, "chunk_cells": None}
    from dataclasses import fields
    assert [f.name for f in fields(GeneBatchHarmonicFit)] == ["means", "stds", "cov", "loglik", "loglik_null", "decrement", "iterations",
                                                              "status", "delta_nu", "delta_nu_stds"]
    x = np.array([0.0, 2.0, 17.5])
    fit = GeneBatchHarmonicFit(means=np.zeros((3, 3)), stds=np.ones((3, 3)), cov=np.zeros((3, 3, 3)), loglik=x / 2, loglik_null=np.zeros(3),
                               decrement=np.zeros(3), iterations=np.zeros(3, np.int32), status=np.zeros(3, np.int32),
                               delta_nu=np.zeros((2, 3)), delta_nu_stds=np.ones((2, 3)))
    assert fit.harmonics == 1 and fit.dof == 2 and np.allclose(fit.lr_stat, x) and np.allclose(fit.p_value, np.exp(-x / 2))


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
    from velocycle_amd import _lib
    from velocycle_amd.containers import Cycle, Phases
    from velocycle_amd.gene_batch import MAX_BATCHES, gene_harmonics_batched
    assert MAX_BATCHES == _lib.VC_GLM_MAX_BATCHES == BC.MAX_BATCHES >= 32
    S = (np.arange(24, dtype=np.float32).reshape(6, 4) % 5) + 1
    xy, n = G.directions(np.linspace(0.1, 6.0, 6)), S.sum(1)
    lab = np.array([0, 1, 0, 1, 2, 2])
    hot = BC.one_hot(lab).T
    # a design that is not one-hot
    for bad in (np.where(np.arange(6)[:, None] == 0, 1.0, hot), hot * 0.5, np.zeros((6, 3)), hot[:5]):
        with pytest.raises(ValueError, match="one-hot|batch design"):
            gene_harmonics_batched(S, xy, n, bad)
    with pytest.raises(ValueError, match="integers"):
        gene_harmonics_batched(S, xy, n, lab + 0.5)
    with pytest.raises(ValueError, match="integers"):
        gene_harmonics_batched(S, xy, n, lab - 1)
    with pytest.raises(ValueError, match="entries"):
        gene_harmonics_batched(S, xy, n, lab[:5])
    # an empty batch: a column of zeros, a label nobody carries
    with pytest.raises(ValueError, match="batch 3 has no cell"):
        gene_harmonics_batched(S, xy, n, np.hstack([hot, np.zeros((6, 1))]))
    with pytest.raises(ValueError, match="batch 1 has no cell"):
        gene_harmonics_batched(S, xy, n, np.array([0, 0, 2, 2, 0, 2]))
    # the prior of the offsets
    for std in (0.0, -1.0, np.inf, np.nan, np.where(np.arange(12).reshape(3, 4) == 5, 0.0, 0.5)):
        with pytest.raises(ValueError, match="std must be finite and > 0"):
            gene_harmonics_batched(S, xy, n, lab, delta_nu_prior=(0.0, std))
    with pytest.raises(ValueError, match="mean must be finite"):
        gene_harmonics_batched(S, xy, n, lab, delta_nu_prior=(np.nan, 0.5))
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        gene_harmonics_batched(S, xy, n, lab, delta_nu_prior=(np.zeros((4, 3)), 0.5))
    with pytest.raises(ValueError, match="every offset needs its prior"):
        gene_harmonics_batched(S, xy, n, lab, delta_nu_prior=None)
    # more batches than the kernel takes
    Nc = MAX_BATCHES + 1
    S2 = np.ones((Nc, 2), np.float32)
    with pytest.raises(ValueError, match="VC_GLM_MAX_BATCHES"):
        gene_harmonics_batched(S2, G.directions(np.linspace(0.1, 6.0, Nc)), np.ones(Nc), np.arange(Nc))
    # the dispersion
    with pytest.raises(ValueError, match="dispersion='mle' is not available with batches.*vc_gene_dispersion"):
        gene_harmonics_batched(S, xy, n, lab, noisemodel="NegativeBinomial", dispersion="mle")
    with pytest.raises(ValueError, match="dispersion"):
        gene_harmonics_batched(S, xy, n, lab, noisemodel="NegativeBinomial", dispersion=0.0)
    # and gene_harmonics' own
    with pytest.raises(NotImplementedError, match="Not implemented yet, sorry"):
        gene_harmonics_batched(S, xy, n, lab, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="harmonics"):
        gene_harmonics_batched(S, xy, n, lab, harmonics=4)
    with pytest.raises(ValueError, match="storage"):
        gene_harmonics_batched(S, xy, n, lab, storage="u8")
    # the containers refuse the same, and what only they can see
    ad, ph = _objects()
    with pytest.raises(NotImplementedError):
        Cycle.from_phases_batch_mle(ph, ad, hot, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="layer"):
        Cycle.from_phases_batch_mle(ph, ad, hot, layer="nope")
    other = type(ph).from_array(ph.phi_xy.values, cell_names=[f"x{i}" for i in range(6)])
    with pytest.raises(ValueError, match="cells"):
        Cycle.from_phases_batch_mle(other, ad, hot)
    with pytest.raises(ValueError, match="genes"):
        Cycle.from_phases_batch_mle(ph, ad, hot, prior=Cycle.trivial_prior(["a", "b", "c", "d"], harmonics=1))
    with pytest.raises(ValueError, match="harmonics"):
        Cycle.from_phases_batch_mle(ph, ad, hot, prior=Cycle.trivial_prior(list(ad.var.index), harmonics=2))
    with pytest.raises(ValueError, match="one-hot"):
        Cycle.from_phases_batch_mle(ph, ad, hot * 2)
    with pytest.raises(ValueError, match="mle"):
        Cycle.from_phases_batch_mle(ph, ad, hot, noisemodel="NegativeBinomial", dispersion="mle")
    cyc = Cycle.from_array(np.zeros((3, 4)), np.ones((3, 4)), gene_names=list(ad.var.index))
    with pytest.raises(ValueError, match="genes"):
        Phases().from_cycle_batch_mle(Cycle.from_array(np.zeros((3, 4)), np.ones((3, 4)), gene_names=list("abcd")), ad, hot, np.zeros((3, 4)))
    with pytest.raises(ValueError, match=r"delta_nu must be \[batches, genes\] = \(3, 4\)"):
        Phases().from_cycle_batch_mle(cyc, ad, hot, np.zeros((4, 3)))
    with pytest.raises(ValueError, match="finite"):
        Phases().from_cycle_batch_mle(cyc, ad, hot, np.full((3, 4), np.nan))
    with pytest.raises(ValueError, match="one-hot"):
        Phases().from_cycle_batch_mle(cyc, ad, hot * 2, np.zeros((3, 4)))
    with pytest.raises(ValueError, match="has no cell"):
        Phases().from_cycle_batch_mle(cyc, ad, np.array([0, 0, 2, 2, 0, 2]), np.zeros((3, 4)))
    with pytest.raises(ValueError, match="bins"):
        Phases().from_cycle_batch_mle(cyc, ad, hot, np.zeros((3, 4)), bins=0)
    with pytest.raises(NotImplementedError):
        Phases().from_cycle_batch_mle(cyc, ad, hot, np.zeros((3, 4)), noisemodel="Lognormal")


def test_batch_labels_and_prior_layout():
    from velocycle_amd.gene_batch import batch_labels, delta_prior
    from velocycle_amd.preprocessing import make_design_matrix
    lab = np.array([2, 0, 1, 1, 2, 0, 0])
    for form in (BC.one_hot(lab).T, torch.tensor(BC.one_hot(lab).T).long(), lab, torch.tensor(lab), lab.astype(np.float64)):
        got, Nb = batch_labels(form, 7)
        assert Nb == 3 and np.array_equal(got, lab) and got.dtype == np.int64
    obs = pd.DataFrame({"batch": ["x", "y", "x", "z"]})
    got, Nb = batch_labels(make_design_matrix(type("A", (), {"obs": obs})()), 4)
    assert Nb == 3 and np.array_equal(got, [0, 1, 0, 2])                      # columns in order of first appearance
    dm, dq = delta_prior((0.25, 0.5), 3, 2)
    assert dm.shape == dq.shape == (2, 3) and dm.dtype == dq.dtype == torch.float64 and bool((dm == 0.25).all()) and bool((dq == 4.0).all())
    mean, std = np.arange(6.0).reshape(3, 2), np.arange(1.0, 7.0).reshape(3, 2)
    dm, dq = delta_prior((mean, std), 3, 2)
    assert np.array_equal(dm.numpy(), mean.T) and np.array_equal(dq.numpy(), 1.0 / std.T ** 2) and dm.is_contiguous()


def test_container_plumbing(monkeypatch):
    from velocycle_amd import gene_batch as GB
    from velocycle_amd import phase_mle as PM
    from velocycle_amd.containers import Cycle, Phases
    from velocycle_amd.utils import torch_fourier_basis
    ad, ph = _objects()
    lab = np.array([1, 0, 2, 0, 1, 2])
    hot = BC.one_hot(lab).T
    seen = {}

    def fake(counts, directions, n_scounts, batches, harmonics=1, a=1, noisemodel="Poisson", dispersion=0.3, **kw):
        seen.update(counts=counts, directions=directions, n_scounts=n_scounts, batches=batches, harmonics=harmonics, a=a,
                    noisemodel=noisemodel, dispersion=dispersion, kw=kw)
        K, Ng = 2 * harmonics + 1, counts.shape[1]
        means = np.arange(K * Ng, dtype=np.float64).reshape(K, Ng)
        return GB.GeneBatchHarmonicFit(means=means, stds=means + 1, cov=np.zeros((Ng, K, K)), loglik=np.ones(Ng), loglik_null=np.zeros(Ng),
                                       decrement=np.zeros(Ng), iterations=np.zeros(Ng, np.int32), status=np.zeros(Ng, np.int32),
                                       delta_nu=np.arange(3 * Ng, dtype=np.float64).reshape(3, Ng) / 10, delta_nu_stds=np.ones((3, Ng)))
    monkeypatch.setattr(GB, "gene_harmonics_batched", fake)
    prior = Cycle.trivial_prior(list(ad.var.index), harmonics=2)
    cyc, fit = Cycle.from_phases_batch_mle(ph, ad, hot, 2, 0.5, "NegativeBinomial", np.full(4, 0.2), delta_nu_prior=(0.1, 0.7), prior=prior,
                                           return_fit=True, chunk_genes=3, tol=1e-8)
    assert isinstance(cyc, Cycle) and list(cyc.means.columns) == list(ad.var.index) and cyc.harmonics == 2
    assert list(cyc.means.index) == ["nu0", "nu1_cos", "nu1_sin", "nu2_cos", "nu2_sin"]
    assert (cyc.means.values == fit.means).all() and (cyc.stds.values == fit.stds).all() and fit.delta_nu.shape == (3, 4)
    assert seen["batches"] is hot and seen["harmonics"] == 2 and seen["a"] == 0.5 and seen["noisemodel"] == "NegativeBinomial"
    assert (seen["dispersion"] == 0.2).all() and seen["kw"]["delta_nu_prior"] == (0.1, 0.7)
    assert (seen["directions"] == ph.phi_xy.values).all() and (np.asarray(seen["n_scounts"]) == ad.obs.n_scounts.values).all()
    assert seen["kw"]["chunk_genes"] == 3 and seen["kw"]["tol"] == 1e-8
    assert (seen["kw"]["prior_means"] == prior.means.values).all() and (seen["kw"]["prior_stds"] == prior.stds.values).all()
    assert (np.asarray(seen["counts"]) == np.asarray(ad.layers["spliced"])).all()
    only = Cycle.from_phases_batch_mle(ph, ad, lab)
    assert isinstance(only, Cycle) and only.harmonics == 1 and seen["kw"]["prior_means"] is None and seen["kw"]["delta_nu_prior"] == (0.0, 0.5)

    # from_cycle_batch_mle: one call of phase_mle per batch, in batch order, on that batch's cells and table; the bins scattered back
    calls = []

    def fake_mle(counts, T, m, noisemodel="Poisson", dispersion=0.3, *, device=None, chunk_cells=None, return_profile=False):
        calls.append(dict(counts=np.asarray(counts), T=T.clone(), m=m.clone(), noisemodel=noisemodel, dispersion=dispersion, device=device,
                          chunk_cells=chunk_cells))
        return (torch.arange(counts.shape[0]) + 10 * len(calls)) % 50, None
    monkeypatch.setattr(PM, "phase_mle", fake_mle)
    cyc1 = Cycle.from_array(np.linspace(-1, 1, 12).reshape(3, 4), np.ones((3, 4)), gene_names=list(ad.var.index))
    dnu = fit.delta_nu
    target = Phases.flat_prior(ad)
    assert target.from_cycle_batch_mle(cyc1, ad, hot, dnu, 0.5, 50, 7.0, "NegativeBinomial", 0.4, device="cuda:0", chunk_cells=128) is None
    assert len(calls) == 3
    phis = (2 * np.pi * torch.arange(0, 1, 1. / 50, dtype=torch.float32))[:50]
    T = torch_fourier_basis(phis, num_harmonics=1).double() @ torch.tensor(cyc1.means.values)
    S = np.asarray(ad.layers["spliced"])
    want = np.empty(6, dtype=np.int64)
    for b, c in enumerate(calls):
        idx = np.flatnonzero(lab == b)
        assert np.array_equal(c["counts"], S[idx]) and torch.equal(c["T"], T + torch.tensor(dnu[b])[None, :])
        assert torch.equal(c["m"], torch.tensor(ad.obs.n_scounts.values[idx].astype(np.float64)) ** 0.5)
        assert c["noisemodel"] == "NegativeBinomial" and c["dispersion"] == 0.4 and c["device"] == "cuda:0" and c["chunk_cells"] == 128
        want[idx] = np.arange(idx.size) + 10 * (b + 1)
    got = target.phi_xy.values.astype(np.float32)
    assert list(target.phi_xy.columns) == list(ad.obs.index)
    assert np.array_equal(got, (7.0 * torch.stack([torch.cos(phis[want]), torch.sin(phis[want])])).numpy())
    fresh = Phases()
    fresh.from_cycle_batch_mle(cyc1, ad, lab, dnu, bins=50)
    assert list(fresh.phi_xy.columns) == list(ad.obs.index) and fresh.phi_xy.shape == (2, 6)


def test_header_declares_and_lib_binds_vc_gene_glm_batch():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert " *   vc_gene_glm_batch " in hdr and "#define VC_ABI_VERSION 2" in hdr
    assert f"#define VC_GLM_MAX_BATCHES {_lib.VC_GLM_MAX_BATCHES}" in hdr and _lib.VC_GLM_MAX_BATCHES >= 32
    decl = re.search(r"\bint vc_gene_glm_batch\(([^;]*)\);", hdr).group(1)
    assert len(_lib.EXPORTS["vc_gene_glm_batch"][1]) == len(decl.split(",")) == 27
    assert decl.rstrip().endswith("void* hip_stream") and "const int64_t* seg_host" in decl
    csrc = os.path.join(ROOT, "velocycle_amd", "csrc")
    read = lambda f: open(os.path.join(csrc, f)).read()                               # noqa: E731
    both = [read(f) for f in ("vc_gene_glm.hip", "vc_gene_glm_batch.hip")]
    solvers = both + [read(f) for f in ("vc_gene_dispersion.hip", "vc_gene_kinetics.hip")]
    # the per-element arithmetic, the count load and the fold are shared through the headers, not copied: by all four per-gene solvers
    for s in solvers:
        assert "__builtin_amdgcn_exp2f((float)(t - tn))" not in s and "__shfl_down" not in s
        assert not re.search(r"\bfloat \w+_count\(", s) and "gene_count<U16>" in s and "gene_fold<" in s
    assert all('#include "vc_gene_glm_math.h"' in s for s in both) and '#include "vc_gene_math.h"' in read("vc_gene_glm_math.h")
    assert all('#include "vc_gene_math.h"' in s for s in solvers[2:])
    assert all("glm_sweep<H, NOISE, U16>" in s for s in both)
    # each shared statement is written once in csrc/
    everything = "".join(read(f) for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")))
    shared = read("vc_gene_math.h")
    for text in ("__builtin_amdgcn_exp2f((float)(t - tn))", "float gene_count(", "void gene_fold(", "void gene_lik(", "int gene_refuse(",
                 "int gene_fail(", "int gene_launched("):
        assert shared.count(text) == 1 == everything.count(text), text
    assert all("gene_exp_f32(" in s for s in (read("vc_gene_glm_math.h"), *solvers[2:]))
    assert "gene_lik<NOISE>" in read("vc_gene_glm_math.h") and solvers[3].count("gene_lik<NOISE>") == 2


def batch_args(**k):
    """Arguments of vc_gene_glm_batch with pointers that are never dereferenced on the device: every call made with them is refused
    before the launch.  seg is host memory and IS read."""
    one = C.c_void_p(64)
    Nb = k.get("Nb", 2)
    seg = k.get("seg", (0, 1, 4))
    seg = (C.c_int64 * len(seg))(*seg) if seg is not None else None
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("noise", 1), k.get("r", None), Nb, seg, k.get("dm", one), k.get("dq", one), k.get("pm", None),
            k.get("pp", None), k.get("tol", 1e-10), k.get("max_iter", 25), k.get("nu", one), k.get("delta", one), k.get("cov", one),
            k.get("dvar", one), k.get("ll", one), k.get("dec", one), k.get("it", one), k.get("st", one), None]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)

    def refused(code=_lib.VC_ERR_ARG, word=b"", **k):
        rc = lib.vc_gene_glm_batch(*batch_args(**k))
        return rc == code and word in lib.vc_last_error(None)
    # a wrong seg
    assert refused(word=b"start at 0", seg=(1, 2, 4))
    assert refused(word=b"end at Nc", seg=(0, 2, 3))
    assert refused(word=b"end at Nc", seg=(0, 2, 5))
    assert refused(word=b"non-decreasing", seg=(0, 5, 4), Nb=2)
    assert refused(word=b"empty segment", seg=(0, 0, 4))
    assert refused(word=b"empty segment", seg=(0, 4, 4))
    assert refused(word=b"null input", seg=None)
    # the number of batches
    assert refused(word=b"VC_GLM_MAX_BATCHES", Nb=0)
    assert refused(word=b"VC_GLM_MAX_BATCHES", Nb=_lib.VC_GLM_MAX_BATCHES + 1, seg=tuple(range(_lib.VC_GLM_MAX_BATCHES + 2)), Nc=_lib.VC_GLM_MAX_BATCHES + 1,
                   stride=_lib.VC_GLM_MAX_BATCHES + 1)
    # every offset needs its prior
    assert refused(word=b"needs its prior", dm=None) and refused(word=b"needs its prior", dq=None)
    # and vc_gene_glm's refusals
    assert refused(_lib.VC_ERR_UNSUPPORTED, b"Lognormal", noise=2)
    for K in (0, 2, 4, 9):
        assert refused(word=b"K must be", K=K)
    for name in ("counts", "basis", "logm"):
        assert refused(word=b"null input", **{name: None}), name
    for name in ("nu", "delta", "cov", "dvar", "ll", "dec", "it", "st"):
        assert refused(word=b"null output", **{name: None}), name
    assert refused(Nc=0) and refused(Ng=0) and refused(word=b"gene_stride", stride=3)
    assert refused(word=b"max_iter", max_iter=0) and refused(word=b"tol", tol=-1e-3) and refused(tol=float("nan"))
    assert refused(word=b"prior of nu", pm=one) and refused(word=b"prior of nu", pp=one)
    assert refused(kind=7) and refused(word=b"r_dev", noise=0) and refused(noise=5)
