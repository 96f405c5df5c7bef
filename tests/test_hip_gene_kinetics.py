"""GPU: vc_gene_kinetics through `gene_kinetics`, the outer fit `velocity_map` and `AngularSpeed.from_kinetics_mle`, held to the
reference and the bars of tests/gene_kinetics_checker.py.  Every test prints the figures it asserts on."""
from dataclasses import fields

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_kinetics_checker as Q
from tests.test_gene_kinetics_cpu import REFUSALS, kin_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import AngularSpeed, Cycle, Phases
from velocycle_amd.gene_kinetics import GeneKineticsFit, gene_kinetics, velocity_map

pytestmark = pytest.mark.gpu


def inputs(p, genes=slice(None)):
    disp = 1.0 / p["r"][genes] if p["r"] is not None else 0.3
    return (p["U"][:, genes].astype(np.float32), Q.directions(p["phis"]), p["n"], p["nu"][genes].T), \
        dict(noisemodel=p["noisemodel"], dispersion=disp)


def design_kw(p):
    return dict(harmonics_w=p["Hw"], condition_design=p["D"])


def run(name, **kw):
    """The inner fit of a case at its own coefficients of the angular speed, on its own design."""
    p = Q.cases()[name]
    args, nb = inputs(p)
    return gene_kinetics(*args, nu_omega=p["nuw"], **design_kw(p), **nb, **kw)


def same_bits(a, b):
    for f in fields(GeneKineticsFit):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), f.name


def assert_within_bars(name, fit, loglik_bar="loglik"):
    bars, worst = Q.bars(), dict(xy=0.0, cov=0.0, loglik=0.0)
    for g, (f64, f32) in enumerate(Q.solved(name)):
        assert fit.status[g] in Q.INTERIOR, (name, g, fit.status[g])
        worst["xy"] = max(worst["xy"], Q.xy_distance(fit.log_gamma[g], fit.log_beta[g], f64))
        worst["cov"] = max(worst["cov"], Q.sym_distance(fit.cov[g], f64["inv"]))
        worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik[g], f64))
        assert fit.iterations[g] <= f32["iterations"] + 2, (name, g, fit.iterations[g], f32["iterations"])
        assert fit.n_clamped[g] == 0 and np.array_equal(fit.stds[:, g], np.sqrt(np.diag(fit.cov[g])))
    print(f"{name}: worst (x, y) {worst['xy']:.3g} se (bar {bars['xy']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), "
          f"objective {worst['loglik']:.3g} eps32 sum |log p| (bar {bars[loglik_bar]:.3g}), steps {fit.iterations.max()}")
    assert worst["xy"] <= bars["xy"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars[loglik_bar]


@pytest.mark.parametrize("Nc,Ng,H,noise", Q.SHAPES)
def test_shapes(Nc, Ng, H, noise):
    name = f"shape_{Nc}_{Ng}_{H}_{noise}"
    fit = run(name)
    assert fit.log_gamma.shape == (Ng,) and fit.cov.shape == (Ng, 2, 2) and fit.score_w.shape == (Ng, 1) and fit.info_w.shape == (Ng, 1, 1)
    assert_within_bars(name, fit)


def test_evaluate_only():
    """The objective, the decrement (both gradients go into it) and n_clamped at five (x, y) per gene, the kernel's start among them;
    the last point clamps cells: n_clamped is the count of a float64 evaluation of the same float32 tables."""
    p = Q.cases()[Q.EVALUATE_CASE]
    Ng = p["U"].shape[1]
    bars, worst = Q.bars(), dict(loglik=0.0, dec=0.0)
    pts = [Q.evaluate_points(p, g) for g in range(Ng)]
    default = run(Q.EVALUATE_CASE, max_iter=1)
    for i in range(len(Q.EVALUATE_AT)):
        start = np.array([[pts[g][i][0] for g in range(Ng)], [pts[g][i][1] for g in range(Ng)]])
        fit = run(Q.EVALUATE_CASE, start=start, evaluate_only=True)
        for g in range(Ng):
            ref, f32 = Q.evaluated()[(i, g)]
            d = dict(loglik=Q.loglik_distance(fit.loglik[g], ref), dec=Q.dec_distance(fit.decrement[g], ref))
            print(f"point {i} gene {g}: objective {d['loglik']:.3g} (restatement {Q.loglik_distance(f32['L'], ref):.3g}), decrement "
                  f"{fit.decrement[g]:.6g} off by {d['dec']:.3g} noise units (restatement {Q.dec_distance(f32['dec'], ref):.3g}), "
                  f"clamped {fit.n_clamped[g]} ({f32['n_clamped']})")
            worst = {key: max(worst[key], d[key]) for key in worst}
            assert fit.status[g] == Q.EVALUATED and fit.iterations[g] == 0 and fit.n_clamped[g] == f32["n_clamped"]
            assert fit.log_gamma[g] == start[0, g] and fit.log_beta[g] == start[1, g]
            assert Q.sym_distance(fit.cov[g], ref["inv"]) <= 1e-4
    assert sum(Q.evaluated()[(4, g)][1]["n_clamped"] for g in range(Ng)) > 0
    # the start the kernel forms itself is the restatement's: one step from it lands where a step from the given start lands
    given = run(Q.EVALUATE_CASE, start=np.array([[pts[g][0][0] for g in range(Ng)], [pts[g][0][1] for g in range(Ng)]]), max_iter=1)
    # (the kernel's sum of e^etaS carries one float32 rounding per cell, eps32 = 1.2e-7, and a Newton step moves with its start)
    assert np.abs(given.log_beta - default.log_beta).max() <= 1e-6 and np.abs(given.log_gamma - default.log_gamma).max() <= 1e-6
    print(f"evaluate-only: worst objective {worst['loglik']:.3g} (bar {bars['ev_loglik']:.3g}), decrement {worst['dec']:.3g} "
          f"(bar {bars['ev_dec']:.3g})")
    assert worst["loglik"] <= bars["ev_loglik"] and worst["dec"] <= bars["ev_dec"]


@pytest.mark.parametrize("name", Q.SCORE_CASES)
def test_score_and_profile_information(name):
    """At the reference's own optimum (evaluate-only), so that both are taken at the same point and the same nuw."""
    p = Q.cases()[name]
    ref = [f64 for f64, _ in Q.solved(name)]
    fit = run(name, start=np.array([[f["x"] for f in ref], [f["y"] for f in ref]]), evaluate_only=True)
    NW = p["W"].shape[0]
    assert fit.score_w.shape == (len(ref), NW) and fit.info_w.shape == (len(ref), NW, NW)
    bars, worst = Q.bars(), dict(score=0.0, info=0.0)
    for g, f64 in enumerate(ref):
        worst["score"] = max(worst["score"], Q.score_distance(fit.score_w[g], f64))
        worst["info"] = max(worst["info"], Q.sym_distance(fit.info_w[g], f64["info"]))
        assert np.array_equal(fit.info_w[g], fit.info_w[g].T)
    print(f"{name}: score {worst['score']:.3g} noise units (bar {bars['score']:.3g}), information {worst['info']:.3g} (bar {bars['info']:.3g})")
    assert worst["score"] <= bars["score"] and worst["info"] <= bars["info"]
    # and the fit's own score and information are those of its own point
    own = run(name)
    assert_within_bars(name, own)
    again = run(name, start=np.stack([own.log_gamma, own.log_beta]), evaluate_only=True)
    assert np.array_equal(own.score_w, again.score_w) and np.array_equal(own.info_w, again.info_w)


@pytest.mark.parametrize("name", Q.LARGE_CASES)
def test_large_counts(name):
    top = Q.cases()[name]["U"].max()
    assert top > 65535 if name == "large_f32" else 2e4 <= top <= 65535
    assert_within_bars(name, run(name), "loglik_large")
    if name == "large_u16":
        same_bits(run(name), run(name, storage="f32"))


def test_confounded_genes_take_the_fisher_step():
    """Genes of the benchmark generator's counts whose observed matrix is positive definite by a hair at the start: the full observed
    step leaves [-30, 30]^2, the Fisher step is taken in its place, and the fit ends where the reference's does."""
    assert sum(f32["fisher_retries"] for _, f32 in Q.solved("confounded")) >= 2
    assert_within_bars("confounded", run("confounded"))


@pytest.mark.parametrize("name", Q.KINK_CASES)
def test_kink_cases_keep_what_holds_there(name):
    """10-20 % of the cells clamped: finite outputs, a documented status, f no lower than at the start, and n_clamped the float64 count
    at the kernel's own point (no cell within 1e-9 of the kink there)."""
    p = Q.cases()[name]
    fit = run(name)
    Nc, Ng = p["U"].shape
    for g in range(Ng):
        k, B, logm, nu, r = Q.gene_inputs(p, g)
        f32 = lambda v: v.astype(np.float32).astype(np.float64)                        # noqa: E731
        at = Q.point64(fit.log_gamma[g], fit.log_beta[g], k, f32(B), f32(logm), nu, f32(p["W"]), p["nuw"], p["noisemodel"], r)
        x0, y0 = Q.start_xy(k, f32(B), f32(logm), nu, f32(p["W"]), p["nuw"])
        f0 = Q.point64(x0, y0, k, f32(B), f32(logm), nu, f32(p["W"]), p["nuw"], p["noisemodel"], r)["f"]
        print(f"{name} gene {g}: status {fit.status[g]}, {fit.iterations[g]} steps, {fit.n_clamped[g]} of {Nc} cells clamped "
              f"({at['n_clamped']}), min |z| {np.abs(at['z']).min():.3g}, f {at['f']:.8g} from {f0:.8g}")
        assert np.abs(at["z"]).min() >= 1e-9
        assert fit.status[g] in (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED)
        assert fit.n_clamped[g] == at["n_clamped"] and at["f"] >= f0
    assert all(np.isfinite(getattr(fit, f.name)).all() for f in fields(fit))
    assert 0.10 <= fit.n_clamped.sum() / (Nc * Ng) <= 0.20


def test_status_cases():
    name = "shape_257_5_1_NegativeBinomial"
    p = Q.cases()[name]
    (U, xy, n, means), nb = inputs(p)
    ref = run(name)
    keep = [0, 1, 3, 4]
    bad = means.copy()
    bad[1, 2] = np.inf
    empty = U.copy()
    empty[:, 2] = 0
    for got in (gene_kinetics(U, xy, n, bad, nu_omega=p["nuw"], **nb), gene_kinetics(empty, xy, n, means, nu_omega=p["nuw"], **nb)):
        assert got.status[2] == Q.NO_DATA and got.iterations[2] == 0 and got.n_clamped[2] == 0
        assert all(np.isnan(getattr(got, f)[2]).all() for f in ("log_gamma", "log_beta", "cov", "loglik", "decrement", "score_w", "info_w"))
        take = lambda fit, f: getattr(fit, f.name)[:, keep] if f.name == "stds" else getattr(fit, f.name)[keep]      # noqa: E731
        assert all(np.array_equal(take(got, f), take(ref, f)) for f in fields(ref))           # the neighbours: bit for bit
    one = run(name, max_iter=1)
    print("max_iter = 1:", one.status, one.iterations)
    assert (one.status == Q.MAX_ITER).all() and (one.iterations == 1).all() and np.isfinite(one.loglik).all()
    mx, sx, my, sy = Q.PRIOR
    f = lambda fit: fit.loglik - 0.5 * ((fit.log_gamma - mx) / sx) ** 2 - 0.5 * ((fit.log_beta - my) / sy) ** 2      # noqa: E731
    assert (f(one) <= f(ref) + 8 * Q.EPS32 * np.abs(ref.loglik)).all()         # one step is below the maximum, up to f's rounding


def test_bit_equal_across_chunks_storage_input_and_repetition():
    p = Q.cases()["score_257_5_2"]
    (U, xy, n, means), nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **design_kw(p), **nb)
    ref = gene_kinetics(U, xy, n, means, **kw)
    for extra in (dict(chunk_genes=1), dict(chunk_genes=2), dict(chunk_genes=5), dict(storage="f32"), dict(storage="u16"), dict()):
        same_bits(ref, gene_kinetics(U, xy, n, means, **kw, **extra))
    same_bits(ref, gene_kinetics(sp.csr_matrix(U), xy, n, means, **kw, chunk_genes=2))
    mkw = dict(**design_kw(p), **nb)
    m = velocity_map(U, xy, n, means, **mkw)
    for extra in (dict(chunk_genes=1), dict(chunk_genes=2), dict(storage="f32"), dict()):
        o = velocity_map(sp.csr_matrix(U) if "storage" in extra else U, xy, n, means, **mkw, **extra)
        same_bits(m.kinetics, o.kinetics)
        assert np.array_equal(m.nu_omega, o.nu_omega) and np.array_equal(m.cov, o.cov) and (m.F, m.dec, m.rounds, m.status) == \
            (o.F, o.dec, o.rounds, o.status)


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_outer_fit(name):
    p = Q.cases()[name]
    m64, m32, _ = Q.outer_solved(name)
    args, nb = inputs(p)
    fit = velocity_map(*args, **design_kw(p), **nb)
    bars = Q.bars()
    v = fit.nu_omega.T.reshape(-1)
    d = v - m64["nuw"]
    dist = float(np.sqrt(d @ m64["J"] @ d))
    std = float(np.abs(fit.stds.T.reshape(-1) / m64["std"] - 1).max())
    z = (v - p["nuw"]) / fit.stds.T.reshape(-1)
    print(f"{name}: nuw {v} +- {fit.stds.T.reshape(-1)}, {dist:.3g} se from the reference's optimum (bar {bars['nuw']:.3g}), stds off by "
          f"{std:.3g} (bar {bars['std']:.3g}), {fit.rounds} rounds (restatement {m32['rounds']}), {z} se from the truth, status "
          f"{fit.status}, dec {fit.dec:.3g}, {fit.n_excluded} excluded, steps per gene {fit.kinetics.iterations.mean():.2f}")
    assert fit.status == "CONVERGED" and fit.n_excluded == 0 and fit.included.all()
    assert dist <= bars["nuw"] and std <= bars["std"] and fit.rounds <= m32["rounds"] + 2
    assert np.abs(z).max() <= 4.0
    assert (fit.kinetics.n_clamped == 0).all() and np.array_equal(fit.stds.T.reshape(-1), np.sqrt(np.diag(fit.cov)))
    assert fit.nu_omega.shape == (2 * p["Hw"] + 1, p["Nx"])


def test_container_path_is_velocity_map():
    p = Q.cases()["score_257_5_2"]
    (U, xy, n, means), nb = inputs(p)
    Nc, Ng = U.shape
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(Nc)])
    ad = AnnDataLite(U * 3, U, gene_names=[f"g{i}" for i in range(Ng)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    cyc = Cycle.from_array(means, np.ones_like(means), gene_names=list(ad.var.index))
    prior = AngularSpeed.trivial_prior(["ctl", "trt"], harmonics=0)
    want = velocity_map(U, xy, n, means, **design_kw(p), **nb, nuw_prior=prior)
    out, fit = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], prior=prior, return_fit=True)
    same_bits(want.kinetics, fit.kinetics)
    assert np.array_equal(out.means.values, want.nu_omega) and np.array_equal(out.stds.values, want.stds) and out.conditions == ["ctl", "trt"]
    assert fit.status == want.status == "CONVERGED" and fit.rounds == want.rounds and fit.F == want.F
    new = fit.to_cycle(cyc)
    assert cyc.log_gammas is None and np.array_equal(new.log_gammas, fit.kinetics.log_gamma) and np.array_equal(new.log_betas, fit.kinetics.log_beta)
    assert new.means.equals(cyc.means) and np.isfinite(new.log_gammas).all()
    alone = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], prior=prior)
    assert alone.means.equals(out.means) and alone.stds.equals(out.stds)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS:
        assert lib.vc_gene_kinetics(*kin_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_kinetics(*kin_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="either omega"):
        gene_kinetics(np.ones((4, 2), np.float32), Q.directions(np.arange(4.0)), np.ones(4), np.zeros((3, 2)))
