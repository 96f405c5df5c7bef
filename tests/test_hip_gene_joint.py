"""GPU: vc_gene_joint through `gene_joint`, the outer fit `velocity_map_joint` and the containers' `from_joint_mle`, held to the
reference and the bars of tests/gene_joint_checker.py.  Every test prints the figures it asserts on."""
import ctypes as C
from dataclasses import fields

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_joint_checker as Q
from tests.test_gene_joint_cpu import REFUSALS, jnt_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import AngularSpeed, Cycle, Phases
from velocycle_amd.gene_harmonics import fourier_basis_from_directions
from velocycle_amd.gene_joint import GeneJointFit, gene_joint, velocity_map_joint
from velocycle_amd.gene_kinetics import gene_kinetics, omega_design
from velocycle_amd.phase_mle import u16_bits

pytestmark = pytest.mark.gpu


def inputs(p, genes=slice(None)):
    disp = 1.0 / p["r"][genes] if p["r"] is not None else 0.3
    return (p["S"][:, genes].astype(np.float32), p["U"][:, genes].astype(np.float32), Q.directions(p["phis"]), p["n"]), \
        dict(harmonics=p["H"], noisemodel=p["noisemodel"], dispersion=disp)


def design_kw(p):
    return dict(harmonics_w=p["Hw"], condition_design=p["D"])


def run(name, **kw):
    """The joint fit of a case at its own coefficients of the angular speed, on its own design."""
    p = Q.cases()[name]
    args, nb = inputs(p)
    return gene_joint(*args, nu_omega=p["nuw"], **design_kw(p), **nb, **kw)


def theta_of(fit, g):
    return np.concatenate([fit.means[:, g], [fit.log_gamma[g], fit.log_beta[g]]])


def start_of(thetas):
    th = np.asarray(thetas)
    return th[:, :-2].T.copy(), th[:, -2].copy(), th[:, -1].copy()


def same_bits(a, b):
    for f in fields(GeneJointFit):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), f.name


def product_tables(p):
    """The float32 tables the product forms from the directions (basis by angle addition), as float64."""
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
    xy = Q.directions(p["phis"])
    return f32(fourier_basis_from_directions(xy, p["H"]).numpy()), f32(np.log(p["n"])), f32(omega_design(xy, p["Hw"], p["D"]))


def point_on_tables(p, g, th):
    """The float64 evaluation of the kernel's own float32 tables at th."""
    B, logm, W = product_tables(p)
    r = float(np.float32(p["r"][g])) if p["r"] is not None else None
    return Q.point64(th, p["S"][:, g], p["U"][:, g], B, logm, W, p["nuw"], p["noisemodel"], r)


def assert_within_bars(name, fit, loglik_bar="loglik"):
    bars, worst = Q.bars(), dict(theta=0.0, cov=0.0, loglik=0.0)
    fits = Q.solved(name)
    Q.assert_kink_free(name, fits)
    for g, (f64, f32) in enumerate(fits):
        if f64["status"] != Q.CONVERGED:
            continue
        assert fit.status[g] in Q.INTERIOR, (name, g, fit.status[g])
        worst["theta"] = max(worst["theta"], Q.theta_distance(theta_of(fit, g), f64))
        worst["cov"] = max(worst["cov"], Q.sym_distance(fit.cov[g], f64["inv"]))
        worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik_S[g], f64, "S"), Q.loglik_distance(fit.loglik_U[g], f64, "U"))
        assert fit.iterations[g] <= bars["steps"], (name, g, fit.iterations[g], bars["steps"])
        assert fit.n_clamped[g] == 0 and np.array_equal(fit.stds[:, g], np.sqrt(np.diag(fit.cov[g])))
    print(f"{name}: worst theta {worst['theta']:.3g} se (bar {bars['theta']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), "
          f"objectives {worst['loglik']:.3g} eps32 sum |log p| (bar {bars[loglik_bar]:.3g}), steps {fit.iterations.max()} "
          f"(restatement's worst {bars['steps']})")
    assert worst["theta"] <= bars["theta"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars[loglik_bar]


@pytest.mark.parametrize("storage", ["u16", "f32"])
@pytest.mark.parametrize("Nc,Ng,H,noise", Q.SHAPES)
def test_shapes(Nc, Ng, H, noise, storage):
    name = f"shape_{Nc}_{Ng}_{H}_{noise}"
    fit = run(name, storage=storage)
    K = 2 * H + 1
    assert fit.means.shape == (K, Ng) and fit.log_gamma.shape == (Ng,) and fit.cov.shape == (Ng, K + 2, K + 2) and fit.stds.shape == (K + 2, Ng)
    assert fit.score_w.shape == (Ng, 1) and fit.info_w.shape == (Ng, 1, 1)
    assert_within_bars(name, fit)


@pytest.mark.parametrize("name", Q.LARGE_CASES)
def test_large_counts(name):
    top = Q.cases()[name]["U"].max()
    assert top > 65535 if name == "large_f32" else 2e4 <= top <= 65535
    assert_within_bars(name, run(name), "loglik_large")
    if name == "large_u16":
        same_bits(run(name, storage="u16"), run(name, storage="f32"))


def test_evaluate_only():
    """Both objectives, the decrement (every gradient goes into it) and n_clamped at five points per gene, the kernel's own start among
    them; the last point clamps cells: n_clamped is the count of a float64 evaluation of the kernel's float32 tables at that point."""
    p = Q.cases()[Q.EVALUATE_CASE]
    Ng = p["U"].shape[1]
    bars, worst = Q.bars(), dict(loglik=0.0, dec=0.0)
    pts = [Q.evaluate_points(p, g) for g in range(Ng)]
    clamped = 0
    for i in range(len(Q.EVALUATE_AT)):
        th = np.array([pts[g][i] for g in range(Ng)])
        fit = run(Q.EVALUATE_CASE, start=start_of(th), evaluate_only=True)
        for g in range(Ng):
            ref, f32 = Q.evaluated()[(i, g)]
            d = dict(loglik=max(Q.loglik_distance(fit.loglik_S[g], ref, "S"), Q.loglik_distance(fit.loglik_U[g], ref, "U")),
                     dec=Q.dec_distance(fit.decrement[g], ref))
            count = point_on_tables(p, g, th[g])["n_clamped"]
            print(f"point {i} gene {g}: objectives {d['loglik']:.3g}, decrement {fit.decrement[g]:.6g} off by {d['dec']:.3g} noise units "
                  f"(restatement {Q.dec_distance(f32['dec'], ref):.3g}), clamped {fit.n_clamped[g]} ({count})")
            worst = {key: max(worst[key], d[key]) for key in worst}
            assert fit.status[g] == Q.EVALUATED and fit.iterations[g] == 0 and fit.n_clamped[g] == count
            assert np.array_equal(theta_of(fit, g), th[g])
            clamped += count if i == 4 else 0
    assert clamped > 0
    # the start the kernel forms itself is the restatement's: one step from it lands where a step from the given start lands
    default, given = run(Q.EVALUATE_CASE, max_iter=1), run(Q.EVALUATE_CASE, start=start_of([pts[g][0] for g in range(Ng)]), max_iter=1)
    # (the kernel's sums of e^etaS and e^logm carry one float32 rounding per cell, eps32 = 1.2e-7, and a Newton step moves with its start)
    assert max(np.abs(theta_of(given, g) - theta_of(default, g)).max() for g in range(Ng)) <= 1e-5
    print(f"evaluate-only: worst objective {worst['loglik']:.3g} (bar {bars['ev_loglik']:.3g}), decrement {worst['dec']:.3g} "
          f"(bar {bars['ev_dec']:.3g})")
    assert worst["loglik"] <= bars["ev_loglik"] and worst["dec"] <= bars["ev_dec"]


def test_unspliced_element_is_vc_gene_kinetics():
    """max_iter == 0: loglik_U and n_clamped are vc_gene_kinetics' evaluate-only outputs at the same (nu, x, y, W, nuw), bit for bit."""
    for name, i in ((Q.EVALUATE_CASE, 4), (Q.EVALUATE_CASE, 2), ("score_257_5_3", 1), ("score_1025_3_2", 3)):
        p = Q.cases()[name]
        (S, U, xy, n), nb = inputs(p)
        th = np.array([Q.evaluate_points(p, g)[i] for g in range(U.shape[1])])
        means, x, y = start_of(th)
        kw = dict(nu_omega=p["nuw"], **design_kw(p), noisemodel=nb["noisemodel"], dispersion=nb["dispersion"], evaluate_only=True)
        jnt = gene_joint(S, U, xy, n, harmonics=p["H"], start=(means, x, y), **kw)
        kin = gene_kinetics(U, xy, n, means, start=np.stack([x, y]), **kw)
        print(f"{name} point {i}: clamped {jnt.n_clamped} {kin.n_clamped}, loglik_U {jnt.loglik_U[0]!r} {kin.loglik[0]!r}")
        assert np.array_equal(jnt.loglik_U, kin.loglik) and np.array_equal(jnt.n_clamped, kin.n_clamped)
        # and the score of nuw: the same element, summed in the same order
        assert np.array_equal(jnt.score_w, kin.score_w)


@pytest.mark.parametrize("name", Q.SCORE_CASES)
def test_score_and_profile_information(name):
    """At the reference's own optimum (evaluate-only), so that both are taken at the same point and the same nuw."""
    p = Q.cases()[name]
    ref = [f64 for f64, _ in Q.solved(name)]
    fit = run(name, start=start_of([f["th"] for f in ref]), evaluate_only=True)
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
    again = run(name, start=(own.means, own.log_gamma, own.log_beta), evaluate_only=True)
    assert np.array_equal(own.score_w, again.score_w) and np.array_equal(own.info_w, again.info_w)


def raw_call(p, genes, stride=None, u16=False, max_iter=40):
    """vc_gene_joint itself on the genes `genes` of a case, rows `stride` counts apart (the padding holds counts that must not be
    read).  Returns (theta, cov, lls, llu, dec, it, st, nc, score, info) as numpy arrays."""
    lib, dev = _lib.load(), torch.device("cuda")
    B, logm, W = (torch.tensor(t, dtype=torch.float32, device=dev).contiguous() for t in product_tables(p))
    Nc, Ng, K, NW = p["U"].shape[0], len(genes), B.shape[0], W.shape[0]
    D, stride = K + 2, stride or Nc

    def block(layer):
        blk = torch.full((Ng, stride), 9.0, dtype=torch.float32, device=dev)
        blk[:, :Nc] = torch.tensor(p[layer][:, genes].T.copy(), dtype=torch.float32, device=dev)
        return u16_bits(blk) if u16 else blk
    S, U = block("S"), block("U")
    pm, pp = Q.prior_of(K)
    f64 = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)     # noqa: E731
    pmt, ppt, prior, nuw = f64(np.tile(pm[:K], (Ng, 1))), f64(np.tile(pp[:K], (Ng, 1))), f64(np.tile(Q.PRIOR, (Ng, 1))), f64(p["nuw"])
    r = torch.tensor(p["r"][genes], dtype=torch.float32, device=dev) if p["r"] is not None else None
    NWH = NW * (NW + 1) // 2
    out = [torch.empty(s, dtype=t, device=dev) for s, t in (((Ng, D), torch.float64), ((Ng, D * (D + 1) // 2), torch.float64),
           ((Ng,), torch.float64), ((Ng,), torch.float64), ((Ng,), torch.float64), ((Ng,), torch.int32), ((Ng,), torch.int32),
           ((Ng,), torch.int32), ((Ng, NW), torch.float64), ((Ng, NWH), torch.float64))]
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                         # noqa: E731
    rc = lib.vc_gene_joint(ptr(S), ptr(U), _lib.VC_COUNTS_U16 if u16 else _lib.VC_COUNTS_F32, Ng, Nc, stride, ptr(B), K, ptr(logm), ptr(W),
                           NW, ptr(nuw), _lib.NOISE[p["noisemodel"]], ptr(r), ptr(pmt), ptr(ppt), ptr(prior), None, 1e-10, max_iter,
                           *[ptr(t) for t in out], None)
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def test_bit_equal_under_stride_cut_storage_and_repetition_in_c():
    p = Q.cases()["score_257_5_3"]
    ref = raw_call(p, [0, 1, 2, 3, 4])
    assert (ref[6] <= Q.ROUNDING).all()
    for other in (raw_call(p, [0, 1, 2, 3, 4]), raw_call(p, [0, 1, 2, 3, 4], stride=300), raw_call(p, [0, 1, 2, 3, 4], stride=258, u16=True),
                  raw_call(p, [0, 1, 2, 3, 4], u16=True)):
        assert all(np.array_equal(a, b) for a, b in zip(ref, other))
    lo, hi = raw_call(p, [0, 1]), raw_call(p, [2, 3, 4], stride=260)
    assert all(np.array_equal(a, np.concatenate([b, c])) for a, b, c in zip(ref, lo, hi))
    # and the Python path on the same problem gives the same numbers
    fit = run("score_257_5_3")
    assert np.array_equal(fit.means.T, ref[0][:, :3]) and np.array_equal(fit.log_beta, ref[0][:, 4]) and np.array_equal(fit.status, ref[6])


def test_bit_equal_across_chunks_storage_input_and_repetition():
    p = Q.cases()["score_257_5_2"]
    (S, U, xy, n), nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **design_kw(p), **nb)
    ref = gene_joint(S, U, xy, n, **kw)
    for extra in (dict(chunk_genes=1), dict(chunk_genes=2), dict(chunk_genes=5), dict(storage="f32"), dict(storage="u16"), dict()):
        same_bits(ref, gene_joint(S, U, xy, n, **kw, **extra))
    same_bits(ref, gene_joint(sp.csr_matrix(S), sp.csr_matrix(U), xy, n, **kw, chunk_genes=2))
    mkw = dict(**design_kw(p), **nb)
    m = velocity_map_joint(S, U, xy, n, **mkw)
    for extra in (dict(chunk_genes=2), dict(storage="f32")):
        o = velocity_map_joint(S, U, xy, n, **mkw, **extra)
        same_bits(m.genes, o.genes)
        assert np.array_equal(m.nu_omega, o.nu_omega) and np.array_equal(m.cov, o.cov) and (m.F, m.dec, m.rounds, m.status) == \
            (o.F, o.dec, o.rounds, o.status)


def test_mixed_storage_takes_float32_for_both_layers():
    """U above 65 535 with S below: both layers are read as float32, and the bits are those of float32 storage."""
    same_bits(run("large_f32"), run("large_f32", storage="f32"))


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_outer_fit(name):
    p = Q.cases()[name]
    m64, m32, _ = Q.outer_solved(name)
    args, nb = inputs(p)
    fit = velocity_map_joint(*args, **design_kw(p), **nb)
    bars = Q.bars()
    v = fit.nu_omega.T.reshape(-1)
    d = v - m64["nuw"]
    dist = float(np.sqrt(d @ m64["J"] @ d))
    std = float(np.abs(fit.stds.T.reshape(-1) / m64["std"] - 1).max())
    z = (v - p["nuw"]) / fit.stds.T.reshape(-1)
    print(f"{name}: nuw {v} +- {fit.stds.T.reshape(-1)}, {dist:.3g} se from the reference's optimum (bar {bars['nuw']:.3g}), stds off by "
          f"{std:.3g} (bar {bars['std']:.3g}), {fit.rounds} rounds (restatement {m32['rounds']}), {z} se from the truth, status "
          f"{fit.status}, dec {fit.dec:.3g}, {fit.n_excluded} excluded, steps per gene {fit.genes.iterations.mean():.2f}")
    assert fit.status == "CONVERGED" and fit.n_excluded == 0 and fit.included.all()
    assert dist <= bars["nuw"] and std <= bars["std"] and fit.rounds == m32["rounds"]
    assert np.abs(z).max() <= 4.0
    assert (fit.genes.n_clamped == 0).all() and np.array_equal(fit.stds.T.reshape(-1), np.sqrt(np.diag(fit.cov)))
    assert fit.nu_omega.shape == (2 * p["Hw"] + 1, p["Nx"])


@pytest.mark.parametrize("name", ["kink_a", "far"])
def test_kink_and_far_start_keep_what_holds_there(name):
    """A kink case (the kinetics checker's kink_a settings) and a far start (nu amplitudes 45, outside the kink-free set): a documented
    status, finite outputs, f no lower than at the start, and n_clamped the float64 count at the kernel's own point."""
    p = Q.cases()[name]
    Nc, Ng = p["U"].shape
    B, logm, W = product_tables(p)
    K = B.shape[0]
    starts = [Q.start_theta(p["S"][:, g], p["U"][:, g], B, logm, W, p["nuw"], Q.prior_of(K)) for g in range(Ng)]
    kw = {}
    if name == "far":
        for th in starts:
            th[1:K] = 45.0
        kw = dict(start=start_of(starts))
    fit = run(name, **kw)
    for g in range(Ng):
        at, f0 = point_on_tables(p, g, theta_of(fit, g)), point_on_tables(p, g, starts[g])["f"]
        print(f"{name} gene {g}: status {fit.status[g]}, {fit.iterations[g]} steps, {fit.n_clamped[g]} of {Nc} cells clamped "
              f"({at['n_clamped']}), f {at['f']:.8g} from {f0:.8g}")
        assert fit.status[g] in (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED)
        assert fit.n_clamped[g] == at["n_clamped"] and at["f"] >= f0
    assert all(np.isfinite(getattr(fit, f.name)).all() for f in fields(fit))


def test_status_cases():
    name = "shape_257_5_1_NegativeBinomial"
    p = Q.cases()[name]
    (S, U, xy, n), nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **nb)
    ref = run(name)
    keep = [0, 1, 3, 4]
    no_S, no_U = S.copy(), U.copy()
    no_S[:, 2], no_U[:, 2] = 0, 0
    stds = np.full((3, 5), 3.0)
    stds[1, 2] = np.nan
    take = lambda fit, f: getattr(fit, f.name)[:, keep] if f.name in ("stds", "means") else getattr(fit, f.name)[keep]      # noqa: E731
    from velocycle_amd import gene_joint as GJ
    fits = [gene_joint(no_S, U, xy, n, **kw), gene_joint(S, no_U, xy, n, **kw)]
    # a NaN prior passes no check_arguments: it reaches the kernel through the problem itself
    basis, logm, r, pm, pp, pr, _ = GJ.check_arguments(S, U, xy, n, **nb)
    pp[2, 1] = np.nan
    prob = GJ._Problem(S, U, basis, logm, r, pm, pp, pr, nb["noisemodel"], None, None, "auto")
    W = torch.as_tensor(omega_design(xy, 0, None)).to(torch.float32).to(prob.dev)
    fits.append(prob.fit(prob.run(W, p["nuw"], None, 1e-10, 40)))
    for got in fits:
        assert got.status[2] == Q.NO_DATA and got.iterations[2] == 0 and got.n_clamped[2] == 0
        assert all(np.isnan(getattr(got, f)[2]).all() for f in ("log_gamma", "log_beta", "cov", "loglik_S", "loglik_U", "decrement", "score_w",
                                                                 "info_w")) and np.isnan(got.means[:, 2]).all()
        assert all(np.array_equal(take(got, f), take(ref, f)) for f in fields(ref))           # the neighbours: bit for bit
    one = run(name, max_iter=1)
    print("max_iter = 1:", one.status, one.iterations)
    assert (one.status == Q.MAX_ITER).all() and (one.iterations == 1).all() and np.isfinite(one.loglik_S).all()
    # a start outside the box, or not finite, falls back to the default start: the default fit's bits
    bad = (ref.means.copy(), ref.log_gamma.copy(), ref.log_beta.copy())
    bad[0][1, 0], bad[1][3] = 51.0, np.nan
    fell = run(name, start=bad)
    for g in (0, 3):
        assert np.array_equal(theta_of(fell, g), theta_of(ref, g)) and fell.iterations[g] == ref.iterations[g]
    assert (fell.iterations[[1, 2, 4]] <= 1).all()                # the others started at the optimum


def test_container_paths():
    p = Q.cases()["score_257_5_2"]
    (S, U, xy, n), nb = inputs(p)
    Nc, Ng = U.shape
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(Nc)])
    ad = AnnDataLite(S, U, gene_names=[f"g{i}" for i in range(Ng)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    prior = AngularSpeed.trivial_prior(["ctl", "trt"], harmonics=0)
    want = velocity_map_joint(S, U, xy, n, **design_kw(p), **nb, nuw_prior=prior)
    out, fit = AngularSpeed.from_joint_mle(None, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], cycle_harmonics=p["H"], prior=prior,
                                           return_fit=True)
    same_bits(want.genes, fit.genes)
    assert np.array_equal(out.means.values, want.nu_omega) and np.array_equal(out.stds.values, want.stds) and out.conditions == ["ctl", "trt"]
    assert fit.status == want.status == "CONVERGED"
    cyc, gfit = Cycle.from_joint_mle(ph, ad, out, p["H"], p["D"], 1, nb["noisemodel"], nb["dispersion"], return_fit=True,
                                     start=(fit.genes.means, fit.genes.log_gamma, fit.genes.log_beta))
    assert (gfit.iterations <= 1).all() and np.allclose(cyc.means.values, fit.genes.means, atol=1e-6)
    assert np.array_equal(cyc.log_gammas, gfit.log_gamma) and np.array_equal(cyc.stds.values, gfit.stds[:2 * p["H"] + 1])
    assert list(cyc.means.columns) == list(ad.var.index)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS:
        assert lib.vc_gene_joint(*jnt_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_joint(*jnt_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="either omega"):
        gene_joint(np.ones((4, 2), np.float32), np.ones((4, 2), np.float32), Q.directions(np.arange(4.0)), np.ones(4))
