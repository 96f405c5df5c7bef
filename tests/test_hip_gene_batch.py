"""GPU: Cycle.from_phases_batch_mle / Phases.from_cycle_batch_mle / velocycle_amd.gene_batch on the HIP kernel vc_gene_glm_batch, judged
by the float64 checker (tests/gene_batch_checker.py: a dense Newton iteration that does not use the block structure) with bars that are
4 x its float32 restatement's own distance from float64 over these very problems (tests/test_gene_batch_cpu.py asserts their cap and
that every reference fit and every restatement ends at its optimum)."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_batch_checker as BC
from tests import gene_glm_checker as G
from tests import mle_checker as MC
from tests import test_cycle_mle_cpu as F
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.gene_batch import gene_harmonics_batched

pytestmark = pytest.mark.gpu
DONE = (G.CONVERGED, G.ROUNDING)
PER_BATCH = ("means", "stds", "delta_nu", "delta_nu_stds")       # genes on the second axis


def run(p, labels=None, counts=None, **kw):
    prior = p["prior"] if p["prior"] is not None else (None, None)
    return gene_harmonics_batched(p["S"].astype(np.float32) if counts is None else counts, G.directions(p["phis"]), p["n"],
                                  p["labels"] if labels is None else labels, harmonics=p["H"], a=p["a"], noisemodel=p["noisemodel"],
                                  dispersion=p["dispersion"] if p["dispersion"] is not None else 0.3, delta_nu_prior=p["dprior"],
                                  prior_means=prior[0], prior_stds=prior[1], **kw)


@lru_cache(maxsize=None)
def fitted(name):
    return run(BC.cases()[name])


def same_bits(a, b, genes=slice(None), other=slice(None)):
    """Every array of two fits, bit for bit (NaN == NaN), on the given genes of each."""
    for f in fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        x, y = (x[:, genes], y[:, other]) if f.name in PER_BATCH else (x[genes], y[other])
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f.name


def assert_within_bars(name, fit, max_iter_over=2, delta_rows=None):
    """Status, iterations and the five yardsticks of every gene against the float64 fits of the case."""
    bars = BC.bars()
    worst = dict.fromkeys(BC.YARDSTICKS, 0.0)
    rows = slice(None) if delta_rows is None else delta_rows
    for g, (f64, n64, f32, n32) in enumerate(BC.solved(name)):
        assert fit.status[g] in DONE, (name, g, fit.status[g])
        assert fit.iterations[g] <= f32["iterations"] + max_iter_over, (name, g, fit.iterations[g], f32["iterations"])
        d = BC.distances(fit.means[:, g], fit.delta_nu[rows, g], fit.stds[:, g], fit.delta_nu_stds[rows, g], fit.loglik[g], fit.lr_stat[g],
                         f64, n64)
        for key in worst:
            worst[key] = max(worst[key], d[key])
    print(f"{name}: worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()) +
          f"; iterations <= {int(fit.iterations.max())}; ROUNDING stops {int((fit.status == G.ROUNDING).sum())}")
    for key in worst:
        assert worst[key] <= bars[key], (name, key, worst[key], bars[key])


@pytest.mark.parametrize("noise,disp", BC.NOISES)
@pytest.mark.parametrize("H", [0, 1, 2])
def test_seven_batches(H, noise, disp):
    """Batches of 1, 63, 64, 65, 255, 256 and 257 cells: less than a wave, a wave and a workgroup, each with one cell less and more."""
    name = f"seven_{H}_{noise}"
    fit = fitted(name)
    p = BC.cases()[name]
    K, Ng, Nb = 2 * H + 1, 5, 7
    assert p["S"].shape == (961, Ng) and tuple(np.bincount(p["labels"])) == BC.SEVEN
    assert fit.means.shape == fit.stds.shape == (K, Ng) and fit.cov.shape == (Ng, K, K) and fit.dof == 2 * H
    assert fit.delta_nu.shape == fit.delta_nu_stds.shape == (Nb, Ng)
    assert np.array_equal(fit.stds, np.sqrt(np.einsum("gii->ig", fit.cov))) and np.array_equal(fit.cov, fit.cov.transpose(0, 2, 1))
    assert_within_bars(name, fit)
    assert (fit.lr_stat >= -BC.bars()["lr"] * G.EPS32 * np.array([s[0]["abs"] for s in BC.solved(name)])).all()
    assert ((fit.p_value >= 0) & (fit.p_value <= 1)).all()
    same_bits(fit, run(p))                                         # a second run
    same_bits(fit, run(p, storage="f32"))
    same_bits(fit, run(p, storage="u16"))
    same_bits(fit, run(p, counts=sp.csr_matrix(p["S"].astype(np.float32))))
    same_bits(fit, run(p, labels=BC.one_hot(p["labels"]).T))      # the one-hot design of the same labels
    for chunk in (1, 2):
        same_bits(fit, run(p, chunk_genes=chunk))


@pytest.mark.parametrize("name", ["one_batch", "one_and_1000", "max_batches", "interleaved", "silent_batch", "nu_prior"])
def test_batch_layouts(name):
    fit = fitted(name)
    p = BC.cases()[name]
    assert fit.delta_nu.shape == (int(p["labels"].max()) + 1, p["S"].shape[1])
    assert_within_bars(name, fit)
    if name == "max_batches":
        assert fit.delta_nu.shape[0] == _lib.VC_GLM_MAX_BATCHES and (np.bincount(p["labels"]) == 8).all()
    if name == "silent_batch":                                    # the prior keeps the offset of the batch without a count finite
        assert (p["S"][p["labels"] == 1, 0] == 0).all() and fit.status[0] in DONE and fit.status[0] != G.UNBOUNDED
        assert -50 < fit.delta_nu[1, 0] < min(fit.delta_nu[0, 0], fit.delta_nu[2, 0]) and np.isfinite(fit.delta_nu_stds).all()
    if name == "interleaved":
        # the permutation: the same cells handed over sorted by batch agree within the bars (another order of the sums), not bit for bit
        assert (np.diff(p["labels"]) < 0).any()
        order = np.argsort(p["labels"], kind="stable")
        q = BC.problem(p["S"][order], p["phis"][order], p["n"][order], p["labels"][order], p["H"], p["noisemodel"], p["dispersion"])
        assert_within_bars(name, run(q))


@pytest.mark.parametrize("noise", [n for n, _ in BC.NOISES])
def test_large_counts(noise):
    for kind in ("u16", "f32"):
        name = f"large_{kind}_{noise}"
        p = BC.cases()[name]
        assert 1e4 <= np.median(p["S"][:, 0]) <= 4e4
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
    S, phis, n, lab = BC.separated()
    Ng = S.shape[1]
    p = BC.problem(S, phis, n, lab, 3, "Poisson")
    fit = run(p)
    assert fit.status[-1] == G.UNBOUNDED, fit.status
    assert np.isfinite(fit.means).all() and np.isfinite(fit.delta_nu).all() and np.isfinite(fit.loglik).all()
    assert set(fit.status[:-1]) <= set(DONE)
    # the neighbours do not know of it
    same_bits(fit, run(BC.problem(S[:, :-1], phis, n, lab, 3, "Poisson")), genes=slice(0, Ng - 1))


def test_relabelling_permutes_the_offsets():
    name = "seven_1_NegativeBinomial"
    p = BC.cases()[name]
    new = np.array([3, 0, 6, 1, 5, 2, 4])                         # batch b is now called new[b]
    fit = run(p, labels=new[p["labels"]])
    assert_within_bars(name, fit, delta_rows=new)                 # row new[b] of the new fit is batch b of the float64 fits


def _glm_on_augmented_design(p, Nb):
    """vc_gene_glm itself on the same penalised problem: the one-hot batch indicators as trailing basis rows, prior precisions on
    those rows only.  Returns nu [Ng, K + Nb] and the status."""
    lib = _lib.load()
    dev = torch.device("cuda")
    S = np.trunc(p["S"])
    Nc, Ng = S.shape
    B = np.vstack([G.basis64(p["phis"], p["H"]), BC.one_hot(p["labels"])])
    Ka = B.shape[0]
    K = Ka - Nb
    pm = np.zeros((Ng, Ka))
    pp = np.zeros((Ng, Ka))
    pm[:, K:], pp[:, K:] = p["dprior"][0], 1.0 / p["dprior"][1] ** 2
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev).contiguous()                   # noqa: E731
    k_d, B_d, logm_d = t(S.T, torch.float32), t(B, torch.float32), t(np.log(p["n"]), torch.float32)
    r_d = torch.full((Ng,), 1.0 / 0.3, dtype=torch.float32, device=dev)
    pm_d, pp_d = t(pm, torch.float64), t(pp, torch.float64)
    nu = torch.empty((Ng, Ka), dtype=torch.float64, device=dev)
    cov = torch.empty((Ng, Ka * (Ka + 1) // 2), dtype=torch.float64, device=dev)
    ll, dec = torch.empty(Ng, dtype=torch.float64, device=dev), torch.empty(Ng, dtype=torch.float64, device=dev)
    it, st = torch.empty(Ng, dtype=torch.int32, device=dev), torch.empty(Ng, dtype=torch.int32, device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                                                                   # noqa: E731
    rc = lib.vc_gene_glm(ptr(k_d), _lib.VC_COUNTS_F32, Ng, Nc, Nc, ptr(B_d), Ka, ptr(logm_d), _lib.NOISE["NegativeBinomial"], ptr(r_d),
                         ptr(pm_d), ptr(pp_d), 1e-10, 25, ptr(nu), ptr(cov), ptr(ll), ptr(dec), ptr(it), ptr(st),
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    return nu.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("H,Nb", [(0, 2), (1, 2), (1, 4), (2, 2)])
def test_two_kernels_one_problem(H, Nb):
    """K + Nb is 3, 5 or 7: a basis vc_gene_glm takes.  Both kernels' optima agree within the sum of their coefficient bars."""
    sizes = (150, 107) if Nb == 2 else (64, 65, 63, 65)
    sim = BC.simulated(sizes, 3, seed=20 + Nb)
    p = BC.problem(sim["S"], sim["phis"], sim["n"], sim["labels"], H, "NegativeBinomial", 0.3, dprior=(0.1, 0.6))
    fit = run(p)
    other, status = _glm_on_augmented_design(p, Nb)
    K = 2 * H + 1
    bar = BC.bars()["coef"] + G.bars()["coef"]
    for g in range(3):
        k, B, lab, logm, r, prior, dprior = BC.gene_inputs(p, g)
        f64 = BC.newton64(k, B, lab, logm, "NegativeBinomial", r, prior, dprior)
        assert f64["status"] == G.CONVERGED and fit.status[g] in DONE and status[g] in DONE
        d = np.concatenate([fit.means[:, g], fit.delta_nu[:, g]]) - other[g]
        dist = float(np.sqrt(max(d @ f64["hess"] @ d, 0.0)))
        print(f"H {H}, Nb {Nb}, gene {g}: the two kernels differ by {dist:.3g} standard errors (bar {bar:.3g})")
        assert dist <= bar, (H, Nb, g, dist, bar)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the device pointers handed over are not device memory."""
    from tests.test_gene_batch_cpu import batch_args
    lib = _lib.load()
    torch.cuda.synchronize()
    assert lib.vc_gene_glm_batch(*batch_args(seg=(0, 0, 4))) == _lib.VC_ERR_ARG and b"empty segment" in lib.vc_last_error(None)
    assert lib.vc_gene_glm_batch(*batch_args(seg=(0, 2, 3))) == _lib.VC_ERR_ARG and b"end at Nc" in lib.vc_last_error(None)
    assert lib.vc_gene_glm_batch(*batch_args(Nb=0)) == _lib.VC_ERR_ARG and b"VC_GLM_MAX_BATCHES" in lib.vc_last_error(None)
    assert lib.vc_gene_glm_batch(*batch_args(dq=None)) == _lib.VC_ERR_ARG and b"needs its prior" in lib.vc_last_error(None)
    assert lib.vc_gene_glm_batch(*batch_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="mle"):
        gene_harmonics_batched(np.ones((4, 2), np.float32), G.directions(np.arange(4.0)), np.ones(4), np.array([0, 1, 0, 1]),
                               noisemodel="NegativeBinomial", dispersion="mle")


def test_container_round_trip():
    """600 cells x 30 genes, three batches that cover different thirds of the cycle, offsets of std 0.5, the true phases in."""
    sim = BC.round_trip()
    S = sim["S"].astype(np.float32)
    Nc, Ng = S.shape
    assert (Nc, Ng) == (600, 30) and sim["dnu"].shape == (3, 30)
    obs = pd.DataFrame({"n_scounts": sim["n"]}, index=[f"c{i}" for i in range(Nc)])
    ad = AnnDataLite(S, S, obs=obs)
    design = BC.one_hot(sim["labels"]).T
    ph = Phases.from_array(G.directions(sim["phis"]), cell_names=list(obs.index))
    cyc, fit = Cycle.from_phases_batch_mle(ph, ad, design, 1, 1, "NegativeBinomial", 0.3, return_fit=True)
    assert set(fit.status) <= set(DONE) and list(cyc.means.columns) == list(ad.var.index)
    assert np.array_equal(cyc.means.values, fit.means) and np.array_equal(cyc.stds.values, fit.stds)
    z = (fit.delta_nu - sim["dnu"]) / fit.delta_nu_stds
    print(f"round trip: simulated offsets within {np.abs(z).max():.2f} standard errors of the estimate")
    assert np.abs(z).max() <= 4.0, z
    # the bias the feature removes: the single-sample fit puts a true sin / cos coefficient outside 4 of its own standard errors
    single = Cycle.from_phases_mle(ph, ad, 1, 1, "NegativeBinomial", 0.3)
    zs = np.abs((single.means.values[1:] - sim["nu"][1:]) / single.stds.values[1:]).max(0)
    zb = np.abs((fit.means[1:] - sim["nu"][1:]) / fit.stds[1:]).max(0)
    print(f"single-sample fit: worst sin / cos z {zs.max():.1f}; batch-aware fit: {zb.max():.1f}")
    assert (zs > 4.0).any()
    # the phases under the fitted offsets: the float64 grid argmax with the offsets
    bins = 100
    target = Phases.flat_prior(ad)
    assert target.from_cycle_batch_mle(cyc, ad, design, fit.delta_nu, 1, bins, 10., "NegativeBinomial", 0.3) is None
    angle = np.arctan2(target.phi_xy.values[1], target.phi_xy.values[0]) % (2 * np.pi)
    chosen = np.rint(angle * bins / (2 * np.pi)).astype(np.int64) % bins
    grid = MC.grid_phases(bins)[torch.as_tensor(chosen)]
    assert np.array_equal(target.phi_xy.values.astype(np.float32), (10. * torch.stack([torch.cos(grid), torch.sin(grid)])).numpy())
    T = MC.table64(fit.means, bins)
    for b in range(3):
        idx = np.flatnonzero(sim["labels"] == b)
        logP, absP = MC.logp64(S[idx], T + torch.tensor(fit.delta_nu[b])[None, :], sim["n"][idx], 1.0, "NegativeBinomial", 0.3)
        j = MC.judge(logP, absP, chosen[idx])
        assert j["regret_ratio"].max() <= F.regret_bar(), (b, j["regret_ratio"].max())
        clear = ~j["excused"]
        assert np.array_equal(chosen[idx][clear], j["best"][clear]), b
    # one batch and no offset: the bits of from_cycle_mle
    a1, a2 = Phases.flat_prior(ad), Phases.flat_prior(ad)
    a1.from_cycle_mle(cyc, ad, 1, bins, 10., "NegativeBinomial", 0.3)
    a2.from_cycle_batch_mle(cyc, ad, np.zeros(Nc, dtype=np.int64), np.zeros((1, Ng)), 1, bins, 10., "NegativeBinomial", 0.3)
    assert a1.phi_xy.values.tobytes() == a2.phi_xy.values.tobytes()
