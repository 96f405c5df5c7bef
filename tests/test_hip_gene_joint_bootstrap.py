"""GPU: the weighted joint fit (vc_gene_joint_weighted) through `gene_joint_weighted` and the C ABI, the cell bootstrap of the joint MAP
angular speed (`velocity_map_joint_bootstrap`) and the containers' `from_joint_mle(bootstrap=)`, held to the references and the bars of
tests/gene_joint_boot_checker.py.  Every test prints the figures it asserts on."""
import ctypes as C
from dataclasses import fields

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gene_joint_boot_checker as X
from tests import gene_joint_checker as Q
from tests.test_gene_joint_bootstrap_cpu import ORDER, REFUSALS, jntw_args
from tests.test_hip_gene_joint import design_kw, inputs, product_tables, raw_call, same_bits, start_of
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import AngularSpeed, Cycle, Phases
from velocycle_amd.gene_joint import GeneJointFit, JointVelocityMapFit, gene_joint, velocity_map_joint
from velocycle_amd.joint_bootstrap import (JointVelocityMapBootstrap, _WeightedProblem, gene_joint_bootstrap, gene_joint_weighted,
                                           velocity_map_joint_bootstrap)
from velocycle_amd.phase_mle import u16_bits

pytestmark = pytest.mark.gpu
OUT = ("theta", "cov", "lls", "llu", "dec", "it", "st", "nc", "score", "info")


def run_w(name, w, **kw):
    """The weighted joint fit of a case at its own coefficients of the angular speed, on its own design."""
    p = Q.cases()[name]
    args, nb = inputs(p)
    return gene_joint_weighted(*args, w, nu_omega=p["nuw"], **design_kw(p), **nb, **kw)


def row_of(fit, b):
    return GeneJointFit(**{f.name: getattr(fit, f.name)[b] for f in fields(GeneJointFit)})


def theta_at(fit, b, g):
    return np.concatenate([fit.means[b][:, g], [fit.log_gamma[b][g], fit.log_beta[b][g]]])


def raw_w(p, genes, w, stride=None, wstride=None, u16=False, max_iter=40, nuw=None, start=None, want_cov=True, prior_prec=None):
    """vc_gene_joint_weighted itself on the genes `genes` of a case under the rows w [R, Nc]: count rows `stride` apart, weight rows
    `wstride` apart (the paddings hold values that must not be read); nuw [NW] or [R, NW]; start None, [Ng, D] or [R, Ng, D].
    Returns a dict of numpy arrays with a leading row axis."""
    lib, dev = _lib.load(), torch.device("cuda")
    B, logm, W = (torch.tensor(t, dtype=torch.float32, device=dev).contiguous() for t in product_tables(p))
    Nc, Ng, K, NW = p["U"].shape[0], len(genes), B.shape[0], W.shape[0]
    D, stride, wstride, R = K + 2, stride or Nc, wstride or Nc, len(w)

    def block(layer):
        blk = torch.full((Ng, stride), 9.0, dtype=torch.float32, device=dev)
        blk[:, :Nc] = torch.tensor(p[layer][:, genes].T.copy(), dtype=torch.float32, device=dev)
        return u16_bits(blk) if u16 else blk
    S, U = block("S"), block("U")
    Wt = torch.full((R, wstride), 5.0, dtype=torch.float32, device=dev)
    Wt[:, :Nc] = torch.tensor(np.asarray(w), dtype=torch.float32, device=dev)
    pm, pp = Q.prior_of(K)
    f64 = lambda v: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)     # noqa: E731
    pmt, prior = f64(np.tile(pm[:K], (Ng, 1))), f64(np.tile(Q.PRIOR, (Ng, 1)))
    ppt = f64(np.tile(pp[:K], (Ng, 1)) if prior_prec is None else prior_prec)
    nuw_t = f64(p["nuw"] if nuw is None else nuw)
    start_t = f64(start) if start is not None else None
    r = torch.tensor(p["r"][genes], dtype=torch.float32, device=dev) if p["r"] is not None else None
    NWH, NHD = NW * (NW + 1) // 2, D * (D + 1) // 2
    shapes = dict(theta=((R, Ng, D), torch.float64), cov=((R, Ng, NHD), torch.float64), lls=((R, Ng), torch.float64),
                  llu=((R, Ng), torch.float64), dec=((R, Ng), torch.float64), it=((R, Ng), torch.int32), st=((R, Ng), torch.int32),
                  nc=((R, Ng), torch.int32), score=((R, Ng, NW), torch.float64), info=((R, Ng, NWH), torch.float64))
    out = {k: torch.full(s, -7, dtype=t, device=dev) for k, (s, t) in shapes.items()}
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                         # noqa: E731
    rc = lib.vc_gene_joint_weighted(ptr(S), ptr(U), _lib.VC_COUNTS_U16 if u16 else _lib.VC_COUNTS_F32, Ng, Nc, stride, ptr(B), K, ptr(logm),
                                    ptr(W), NW, ptr(nuw_t), NW if nuw_t.ndim == 2 else 0, _lib.NOISE[p["noisemodel"]], ptr(r), ptr(pmt),
                                    ptr(ppt), ptr(prior), ptr(Wt), R, wstride, ptr(start_t),
                                    (Ng * D if start_t.ndim == 3 else 0) if start_t is not None else 0, 1e-10, max_iter,
                                    *[ptr(out[k]) if (k != "cov" or want_cov) else None for k in OUT], None)
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def same(a, b, keys=OUT):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def rows_of(o, sel):
    return {k: v[sel] for k, v in o.items()}


def genes_of(o, sel):
    return {k: v[:, sel] for k, v in o.items()}


def cat(parts, axis):
    return {k: np.concatenate([q[k] for q in parts], axis) for k in OUT}


# ---------------------------------------------------------------------------------------------------------------- unit weights
@pytest.mark.parametrize("name", X.PAIR_CASES)
def test_unit_weights_reproduce_vc_gene_joint(name):
    """A table of ones, R = 1, strides 0: every output of vc_gene_joint bit for bit, from the default start, through Python (the
    full log-likelihoods' constants included) and through the C ABI."""
    p = Q.cases()[name]
    Nc, Ng = p["U"].shape
    same_bits(run_w(name, np.ones(Nc)), gene_joint(*inputs(p)[0], nu_omega=p["nuw"], **design_kw(p), **inputs(p)[1]))
    plain = raw_call(p, list(range(Ng)))
    got = raw_w(p, list(range(Ng)), np.ones((1, Nc)))
    for k, a in zip(OUT, plain):
        assert np.array_equal(got[k][0], a, equal_nan=True), (name, k)
    assert (got["st"] != -7).all()


def test_unit_weights_from_a_start_and_evaluate_only():
    name = "score_257_5_3"
    p = Q.cases()[name]
    args, nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **design_kw(p), **nb)
    start = start_of([f64["th"] + 0.01 for f64, _ in Q.solved(name)])
    ones = np.ones(p["U"].shape[0])
    for extra in (dict(start=start), dict(start=start, evaluate_only=True), dict(start=start, max_iter=1), dict(storage="f32")):
        same_bits(gene_joint_weighted(*args, ones, **kw, **extra), gene_joint(*args, **kw, **extra))
    two = gene_joint_weighted(*args, np.ones((2, len(ones))), **kw)
    assert two.means.shape == (2, 3, 5) and two.cov.shape == (2, 5, 5, 5) and two.status.shape == (2, 5) and two.info_w.shape == (2, 5, 3, 3)
    same_bits(row_of(two, 0), gene_joint(*args, **kw))
    same_bits(row_of(two, 1), gene_joint(*args, **kw))


# ---------------------------------------------------------------------------------------------------------------- the bars
def check_pairs(name, solved, w, start, steps_key):
    """theta, the inverse, both objectives and the steps of every pair of a case against the expansion's reference; for a score
    case the score and the profile information at the reference's own optimum."""
    p = Q.cases()[name]
    bars = X.bars()
    worst = dict(theta=0.0, cov=0.0, loglik=0.0, score=0.0, info=0.0)
    rows = solved(name)
    fit = run_w(name, w, **({} if start is None else dict(start=start_of(start))))
    for b, row in enumerate(rows):
        for g, s in enumerate(row):
            if s is None:
                assert fit.status[b][g] == Q.NO_DATA and np.isnan(theta_at(fit, b, g)).all() and np.isnan(fit.loglik_S[b][g]), (name, b, g)
                continue
            f64 = s[0]
            assert fit.status[b][g] in Q.INTERIOR and fit.n_clamped[b][g] == 0, (name, b, g, fit.status[b][g])
            assert fit.iterations[b][g] <= bars[steps_key] + 1, (name, b, g, fit.iterations[b][g])
            worst["theta"] = max(worst["theta"], Q.theta_distance(theta_at(fit, b, g), f64))
            worst["cov"] = max(worst["cov"], Q.sym_distance(fit.cov[b][g], f64["inv"]))
            worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik_S[b][g], f64, "S"), Q.loglik_distance(fit.loglik_U[b][g], f64, "U"))
        if name in Q.SCORE_CASES:                                            # at the reference's own optimum of this row
            at = run_w(name, w[b], start=start_of([s[0]["th"] for s in row]), evaluate_only=True)
            for g, s in enumerate(row):
                worst["score"] = max(worst["score"], Q.score_distance(at.score_w[g], s[0]))
                worst["info"] = max(worst["info"], Q.sym_distance(at.info_w[g], s[0]["info"]))
    key = "loglik_large" if name in Q.LARGE_CASES else "loglik"
    print(f"{name}: theta {worst['theta']:.3g} se (bar {bars['theta']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), objectives "
          f"{worst['loglik']:.3g} (bar {bars[key]:.3g}), score {worst['score']:.3g} (bar {bars['score']:.3g}), information {worst['info']:.3g} "
          f"(bar {bars['info']:.3g}), steps {fit.iterations.max()} (restatement's worst {bars[steps_key]})")
    assert worst["theta"] <= bars["theta"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars[key]
    assert worst["score"] <= bars["score"] and worst["info"] <= bars["info"]


@pytest.mark.parametrize("name", X.PAIR_CASES)
def test_bars_warm_start(name):
    check_pairs(name, X.solved_warm, X.weights(name), X.warm_starts(name), "steps_warm")


@pytest.mark.parametrize("name", list(X.DEFAULT_SEEDS))
def test_bars_default_start(name):
    check_pairs(name, X.solved_default, X.weights(name, X.DEFAULT_SEEDS[name]), None, "steps_default")


def test_evaluate_only_under_weights():
    """max_iter == 0 at EVALUATE_AT's points under the case's three rows: both objectives and the decrement against the expansion's
    float64 evaluation; the last point clamps cells, and n_clamped is the float64 count over the cells with w > 0."""
    name = Q.EVALUATE_CASE
    p, Wt = Q.cases()[name], X.weights(name)
    Ng = p["U"].shape[1]
    B, logm, W = product_tables(p)
    bars, worst, clamped = X.bars(), dict(loglik=0.0, dec=0.0), 0
    for b, w in enumerate(Wt):
        for i in range(len(Q.EVALUATE_AT)):
            th = np.array([X.evaluated()[(b, i, g)][2] for g in range(Ng)])
            fit = run_w(name, w, start=start_of(th), evaluate_only=True)
            for g in range(Ng):
                ref = X.evaluated()[(b, i, g)][0]
                worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik_S[g], ref, "S"), Q.loglik_distance(fit.loglik_U[g], ref, "U"))
                worst["dec"] = max(worst["dec"], Q.dec_distance(fit.decrement[g], ref))
                r = float(np.float32(p["r"][g]))
                count = X.weighted_point64(th[g], p["S"][:, g], p["U"][:, g], B, logm, W, p["nuw"], w, p["noisemodel"], r)["n_clamped"]
                assert fit.status[g] == Q.EVALUATED and fit.iterations[g] == 0 and fit.n_clamped[g] == count, (b, i, g, fit.n_clamped[g], count)
                clamped += count if i == 4 else 0
    print(f"evaluate-only under weights: objectives {worst['loglik']:.3g} (bar {bars['ev_loglik']:.3g}), decrement {worst['dec']:.3g} "
          f"(bar {bars['ev_dec']:.3g}), clamped cells at the last point {clamped}")
    assert clamped > 0 and worst["loglik"] <= bars["ev_loglik"] and worst["dec"] <= bars["ev_dec"]


def test_non_integer_weights():
    """Uniform (0, 3) float32 weights, 2 x 257, from the warm start, against the written-out weighted formulas in float64."""
    name = X.UNIFORM_CASE
    bars, worst = X.bars(), dict(theta=0.0, cov=0.0, loglik=0.0)
    fit = run_w(name, X.uniform_weights(), start=start_of(X.warm_starts(name)))
    for b, row in enumerate(X.solved_uniform()):
        for g, ref in enumerate(row):
            assert fit.status[b][g] in Q.INTERIOR and fit.n_clamped[b][g] == 0
            worst["theta"] = max(worst["theta"], Q.theta_distance(theta_at(fit, b, g), ref))
            worst["cov"] = max(worst["cov"], Q.sym_distance(fit.cov[b][g], ref["inv"]))
            worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik_S[b][g], ref, "S"), Q.loglik_distance(fit.loglik_U[b][g], ref, "U"))
    print(f"non-integer weights: theta {worst['theta']:.3g} (bar {bars['theta']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), "
          f"objectives {worst['loglik']:.3g} (bar {bars['loglik']:.3g})")
    assert worst["theta"] <= bars["theta"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars["loglik"]


# ---------------------------------------------------------------------------------------------------------------- rows and cuts
def test_rows_cuts_storage_and_strides_in_c():
    p = Q.cases()["score_257_5_3"]
    w = X.weights("score_257_5_3")
    genes = [0, 1, 2, 3, 4]
    ref = raw_w(p, genes, w)
    assert (ref["st"] <= Q.ROUNDING).all()
    same(ref, raw_w(p, genes, w))                                            # repetition
    same(ref, cat([raw_w(p, genes, w[b:b + 1]) for b in range(3)], 0))       # 3 rows against three 1-row calls
    same(ref, cat([raw_w(p, [0, 1], w), raw_w(p, [2, 3, 4], w)], 1))         # five genes against calls of 2 and 3
    same(ref, raw_w(p, genes, w, u16=True))
    same(ref, raw_w(p, genes, w, stride=258, u16=True))
    same(ref, raw_w(p, genes, w, stride=300))
    same(ref, raw_w(p, genes, w, wstride=257 + 3))
    no_cov = raw_w(p, genes, w, want_cov=False)
    same(ref, no_cov, [k for k in OUT if k != "cov"])
    assert (no_cov["cov"] == -7).all()                                       # NULL: not stored


def test_chunks_storage_and_input_through_python():
    import scipy.sparse as sp
    name = "score_257_5_2"
    p, w = Q.cases()[name], X.weights(name)
    (S, U, xy, n), nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **design_kw(p), **nb)
    ref = gene_joint_weighted(S, U, xy, n, w, **kw)
    for extra in (dict(chunk_genes=1), dict(chunk_genes=2), dict(chunk_genes=5), dict(storage="f32"), dict(storage="u16")):
        same_bits(ref, gene_joint_weighted(S, U, xy, n, w, **kw, **extra))
    same_bits(ref, gene_joint_weighted(sp.csr_matrix(S), sp.csr_matrix(U), xy, n, w, **kw, chunk_genes=2))
    same_bits(row_of(ref, 1), gene_joint_weighted(S, U, xy, n, w[1], **kw))
    # mixed storage: U above 65 535 with S below takes float32 for both layers
    wl = X.weights("large_f32")
    same_bits(run_w("large_f32", wl), run_w("large_f32", wl, storage="f32"))


def test_per_row_nuw_and_start():
    """Row b of a call with per-row coefficients and starts equals the 1-row call at its own."""
    name = "score_257_5_2"
    p, w = Q.cases()[name], X.weights(name)
    genes = [0, 1, 2, 3, 4]
    nuw = np.stack([p["nuw"] * (1.0 + 0.05 * b) for b in range(3)])
    base = np.array(X.warm_starts(name))
    start = np.stack([base + 0.01 * (b + 1) for b in range(3)])
    start[2, 1, 0] = np.nan                                                  # this pair falls back to the default start
    ref = raw_w(p, genes, w, nuw=nuw, start=start)
    assert (ref["st"] != -7).all()
    for b in range(3):
        same(rows_of(ref, slice(b, b + 1)), raw_w(p, genes, w[b:b + 1], nuw=nuw[b], start=start[b]))
    assert not np.array_equal(ref["theta"][0], ref["theta"][1])
    same(genes_of(rows_of(ref, slice(2, 3)), [1]), raw_w(p, [1], w[2:3], nuw=nuw[2]))      # the default start's bits
    shared = raw_w(p, genes, w, nuw=nuw[1], start=start[1])
    same(rows_of(shared, slice(1, 2)), rows_of(ref, slice(1, 2)))


def test_more_genes_than_one_launch():
    """Ng = 65 537 at Nc = 2, R = 2: the second launch (genes 65 535 and 65 536) against a call cut at 65 535."""
    rng = np.random.default_rng(5)
    Ng, Nc = 65537, 2
    p = dict(S=rng.poisson(20.0, (Nc, Ng)).astype(np.float64) + 1, U=rng.poisson(5.0, (Nc, Ng)).astype(np.float64) + 1,
             phis=np.array([0.3, 2.1]), n=np.array([1.0, 1.2]), H=1, Hw=0, D=None, nuw=np.array([0.3]), r=None, noisemodel="Poisson")
    w = np.array([[1.0, 2.0], [3.0, 1.0]])
    whole = raw_w(p, np.arange(Ng), w, max_iter=3)
    assert (whole["st"] != -7).all() and np.isfinite(whole["theta"]).all()
    same(genes_of(whole, slice(0, 65535)), raw_w(p, np.arange(65535), w, max_iter=3))
    same(genes_of(whole, slice(65535, Ng)), raw_w(p, np.arange(65535, Ng), w, max_iter=3))


def test_planted_rows_end_no_data_and_touch_no_neighbour():
    name = "shape_257_5_1_NegativeBinomial"
    p = Q.cases()[name]
    genes = [0, 1, 2, 3, 4]
    w = X.weights(name, rows=4)
    ref = raw_w(p, genes, w)
    planted = w.copy()
    planted[1] = 0.0                                                         # a row of zeros
    planted[2, 17] = np.nan                                                  # a NaN weight
    planted[3, p["U"][:, 2] > 0] = 0.0                                       # row 3 empties the unspliced layer of gene 2
    got = raw_w(p, genes, planted)
    lost = np.zeros((4, 5), bool)
    lost[1], lost[2], lost[3, 2] = True, True, True
    assert (got["st"][lost] == Q.NO_DATA).all() and (got["it"][lost] == 0).all() and (got["nc"][lost] == 0).all()
    for k in ("theta", "cov", "lls", "llu", "dec", "score", "info"):
        assert np.isnan(got[k][lost]).all(), k
    same(rows_of(got, slice(0, 1)), rows_of(ref, slice(0, 1)))               # the neighbours: bit for bit
    alone = raw_w(p, genes, planted[3:4])
    same(rows_of(got, slice(3, 4)), alone)
    assert (got["st"][3, [0, 1, 3, 4]] <= Q.ROUNDING).all() and np.isfinite(got["theta"][3, [0, 1, 3, 4]]).all()
    # a start does not rescue a pair without data
    start = np.array(X.warm_starts(name))
    assert (raw_w(p, genes, planted[1:2], start=start)["st"] == Q.NO_DATA).all()
    # a non-finite prior ends NO_DATA in every row of that gene only
    pp = np.tile(Q.prior_of(3)[1][:3], (5, 1))
    pp[2, 1] = np.nan
    bad = raw_w(p, genes, w, prior_prec=pp)
    assert (bad["st"][:, 2] == Q.NO_DATA).all() and np.isnan(bad["theta"][:, 2]).all()
    same(genes_of(bad, [0, 1, 3, 4]), genes_of(ref, [0, 1, 3, 4]))


def test_kink_a_under_weights():
    """The kink case under its weights: every pair ends in a documented status within max_iter steps, with finite outputs, f not lower
    than at the start, and n_clamped the float64 count over the cells with w > 0 at the kernel's own point."""
    p = Q.cases()["kink_a"]
    Nc, Ng = p["U"].shape
    w = X.weights("kink_a")
    B, logm, W = product_tables(p)
    fit = run_w("kink_a", w)
    for b in range(len(w)):
        for g in range(Ng):
            args = (p["S"][:, g], p["U"][:, g], B, logm, W, p["nuw"], w[b], p["noisemodel"], None)
            start = X.weighted_start(*args[:7], Q.prior_of(3))
            at, f0 = X.weighted_point64(theta_at(fit, b, g), *args), X.weighted_point64(start, *args)["f"]
            print(f"kink_a row {b} gene {g}: status {fit.status[b][g]}, {fit.iterations[b][g]} steps, {fit.n_clamped[b][g]} clamped "
                  f"({at['n_clamped']}), f {at['f']:.8g} from {f0:.8g}")
            assert fit.status[b][g] in (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED) and fit.iterations[b][g] <= 40
            assert fit.n_clamped[b][g] == at["n_clamped"] and at["f"] >= f0 - 1e-9 * abs(f0)
    assert all(np.isfinite(getattr(fit, f.name)).all() for f in fields(fit))


# ---------------------------------------------------------------------------------------------------------------- the outer fit
def fit_from_reference(p, m):
    """The `JointVelocityMapFit` that holds the reference's full-data optimum: the bootstrap's warm start."""
    th = np.array([f["th"] for f in m["fits"]])
    Ng, K, NW, z = th.shape[0], th.shape[1] - 2, len(m["nuw"]), np.zeros(th.shape[0])
    genes = GeneJointFit(means=th[:, :K].T.copy(), log_gamma=th[:, K].copy(), log_beta=th[:, K + 1].copy(),
                         cov=np.array([f["inv"] for f in m["fits"]]), stds=np.sqrt(np.array([np.diag(f["inv"]) for f in m["fits"]])).T.copy(),
                         loglik_S=z, loglik_U=z, decrement=z, iterations=np.zeros(Ng, np.int32), status=np.zeros(Ng, np.int32),
                         n_clamped=np.zeros(Ng, np.int32), score_w=np.zeros((Ng, NW)), info_w=np.zeros((Ng, NW, NW)))
    Nhw = 2 * p["Hw"] + 1
    table = lambda v: np.ascontiguousarray(v.reshape(p["Nx"], Nhw).T)           # noqa: E731
    return JointVelocityMapFit(nu_omega=table(m["nuw"]), stds=table(m["std"]), cov=m["cov"], F=m["F"], dec=m["dec"], rounds=m["rounds"],
                               status=m["status"], n_excluded=0, included=np.ones(Ng, bool), genes=genes)


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_outer_bootstrap_against_the_expansion(name):
    p = Q.cases()[name]
    args, nb = inputs(p)
    full = fit_from_reference(p, Q.outer_solved(name)[0])
    w = X.weights(name, rows=X.OUTER_ROWS)
    bs = velocity_map_joint_bootstrap(*args, **design_kw(p), **nb, weights=w, fit=full, keep_genes=True, return_weights=True)
    bars = X.bars()
    assert isinstance(bs, JointVelocityMapBootstrap) and bs.fit is full and np.array_equal(bs.weights, w.astype(np.float32))
    assert bs.nu_omega_replicates.shape == (2, 2 * p["Hw"] + 1, p["Nx"]) and bs.theta_replicates.shape == (2, p["U"].shape[1], 5)
    for b, (m64, m32, _) in enumerate(X.outer_solved(name)):
        v = bs.nu_omega_replicates[b].T.reshape(-1)
        d = v - m64["nuw"]
        dist = float(np.sqrt(d @ m64["J"] @ d))
        print(f"{name} row {b}: nuw {v}, {dist:.3g} se from the reference (bar {bars['nuw']:.3g}), {bs.rounds[b]} rounds (restatement "
              f"{m32['rounds']}), status {bs.status[b]}, dec {bs.dec[b]:.3g}, {bs.n_excluded[b]} excluded, "
              f"{np.abs(v - full.nu_omega.T.reshape(-1)) / full.stds.T.reshape(-1)} se from the full fit")
        assert bs.status[b] == "CONVERGED" and bs.n_excluded[b] == 0 and bs.gene_included[b].all()
        assert dist <= bars["nuw"] and bs.rounds[b] == m32["rounds"]
        # the replicate's own Laplace stds: the device's profile information J at its optimum against the reference's
        std = float(np.abs(bs.laplace_stds[b].T.reshape(-1) / m64["std"] - 1).max())
        print(f"  Laplace stds {bs.laplace_stds[b].T.reshape(-1)} off by {std:.3g} (bar {bars['std']:.3g})")
        assert std <= bars["std"]
        # the genes sit at the replicate's own nuw: they are reported, the bar is the pairs' (test_bars_warm_start)
        print("  genes' worst distance from the reference's, se:",
              max(Q.theta_distance(bs.theta_replicates[b, g], f) for g, f in enumerate(m64["fits"])))
    assert bs.ok.all() and np.isfinite(bs.stds).all() and np.isfinite(bs.gene_stds()).all()


def test_replicates_do_not_know_of_each_other_and_ones_reproduce_the_fit():
    name = "outer_1500_30"
    p = Q.cases()[name]
    args, nb = inputs(p)
    kw = dict(**design_kw(p), **nb)
    full = velocity_map_joint(*args, **kw)
    four = velocity_map_joint_bootstrap(*args, **kw, n_boot=4, seed=3, fit=full, keep_genes=True, return_weights=True)
    two = velocity_map_joint_bootstrap(*args, **kw, n_boot=2, seed=3, fit=full, keep_genes=True, return_weights=True, chunk_genes=7)
    for f in ("nu_omega_replicates", "status", "rounds", "n_excluded", "F", "dec", "laplace_stds", "theta_replicates", "gene_status", "gene_included",
              "weights"):
        assert np.array_equal(getattr(four, f)[:2], getattr(two, f)), f
    print("statuses", four.status, "rounds", four.rounds, "contrast sd", four.contrast_std(0, 1))
    assert four.ok.all() and four.nu_omega_replicates.std(0).min() > 0
    # the drawn weights are the other bootstraps' for the same seed
    from velocycle_amd.gene_bootstrap import draw_weights, gene_harmonics_bootstrap
    assert np.array_equal(four.weights, draw_weights(4, p["U"].shape[0], 3, torch.device("cuda")).cpu().numpy())
    hb = gene_harmonics_bootstrap(args[0], args[2], args[3], harmonics=1, n_boot=4, seed=3, return_weights=True)
    assert np.array_equal(four.weights, hb.weights)
    # a row of ones from the cold start is velocity_map_joint itself
    ones = velocity_map_joint_bootstrap(*args, **kw, weights=np.ones((1, p["U"].shape[0])), fit=full, warm_start=False, keep_genes=True)
    assert np.array_equal(ones.nu_omega_replicates[0], full.nu_omega) and ones.F[0] == full.F and ones.rounds[0] == full.rounds
    assert ones.status[0] == full.status and ones.dec[0] == full.dec and np.array_equal(ones.laplace_stds[0], full.stds)
    th = np.concatenate([full.genes.means.T, full.genes.log_gamma[:, None], full.genes.log_beta[:, None]], 1)
    assert np.array_equal(ones.theta_replicates[0], th) and np.array_equal(ones.gene_status[0], full.genes.status)
    # gene_stds over the replicates, and the cycle that carries them
    sd = four.gene_stds()
    assert sd.shape == (5, p["U"].shape[1]) and np.isfinite(sd).all() and (sd > 0).all()
    cyc = four.to_cycle([f"g{i}" for i in range(p["U"].shape[1])])
    assert np.array_equal(cyc.stds.values, sd[:3]) and np.array_equal(cyc.means.values, full.genes.means)


def test_a_gene_emptied_in_one_replicate_is_excluded_there_only():
    """Gene 4 has unspliced counts in the first 200 cells only; replicate 1 draws weight 0 for those."""
    name = "outer_1500_30"
    p = Q.cases()[name]
    (S, U, xy, n), nb = inputs(p)
    U = U.copy()
    U[200:, 4] = 0
    args = (S, U, xy, n)
    kw = dict(**design_kw(p), **nb)
    full = velocity_map_joint(*args, **kw)
    assert full.included[4] and full.status == "CONVERGED"
    w = X.weights(name, rows=2)
    ref = velocity_map_joint_bootstrap(*args, **kw, weights=w, fit=full, keep_genes=True)
    planted = w.copy()
    planted[1, :200] = 0.0
    got = velocity_map_joint_bootstrap(*args, **kw, weights=planted, fit=full, keep_genes=True)
    assert list(got.n_excluded) == [0, 1] and not got.gene_included[1, 4] and got.gene_included[0].all() and got.gene_status[1, 4] == Q.NO_DATA
    assert got.status[1] == "CONVERGED" and np.isfinite(got.nu_omega_replicates[1]).all()
    for f in ("nu_omega_replicates", "F", "dec", "rounds", "theta_replicates"):
        assert np.array_equal(getattr(got, f)[0], getattr(ref, f)[0]), f
    sd = got.gene_stds()
    assert np.isnan(sd[:, 4]).all() and np.isfinite(np.delete(sd, 4, 1)).all()      # one replicate left for gene 4


def test_container_paths():
    p = Q.cases()["score_257_5_2"]
    (S, U, xy, n), nb = inputs(p)
    Nc, Ng = U.shape
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(Nc)])
    ad = AnnDataLite(S, U, gene_names=[f"g{i}" for i in range(Ng)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    prior = AngularSpeed.trivial_prior(["ctl", "trt"], harmonics=0)
    plain, pfit = AngularSpeed.from_joint_mle(None, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], cycle_harmonics=p["H"], prior=prior,
                                              return_fit=True)
    out, fit = AngularSpeed.from_joint_mle(None, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], cycle_harmonics=p["H"], prior=prior,
                                           return_fit=True, bootstrap=6, bootstrap_seed=2)
    assert pfit.bootstrap is None and out.means.equals(plain.means) and out.stds.equals(plain.stds)
    same_bits(pfit.genes, fit.genes)
    want = velocity_map_joint_bootstrap(S, U, xy, n, **design_kw(p), **nb, nuw_prior=prior, n_boot=6, seed=2, fit=pfit, keep_genes=True)
    bs = fit.bootstrap
    assert isinstance(bs, JointVelocityMapBootstrap) and np.array_equal(bs.nu_omega_replicates, want.nu_omega_replicates)
    assert np.array_equal(bs.theta_replicates, want.theta_replicates, equal_nan=True) and list(bs.status) == list(want.status)
    print("container: statuses", bs.status, "contrast sd", bs.contrast_std(0, 1), "Laplace stds", out.stds.values)
    cyc0, g0 = Cycle.from_joint_mle(ph, ad, out, p["H"], p["D"], 1, nb["noisemodel"], nb["dispersion"], return_fit=True)
    cyc, g = Cycle.from_joint_mle(ph, ad, out, p["H"], p["D"], 1, nb["noisemodel"], nb["dispersion"], return_fit=True, bootstrap=5)
    same_bits(g0, g)
    assert g0.bootstrap is None and cyc.means.equals(cyc0.means) and np.array_equal(cyc.log_gammas, cyc0.log_gammas)
    assert np.array_equal(cyc.stds.values, g.bootstrap.gene_stds()[:2 * p["H"] + 1]) and not cyc.stds.equals(cyc0.stds)
    nuw = np.ascontiguousarray(out.means.values.T).reshape(-1)
    want = gene_joint_bootstrap(S, U, xy, n, harmonics=p["H"], **{k: v for k, v in nb.items() if k != "harmonics"}, nu_omega=nuw,
                                **design_kw(p), n_boot=5, fit=g0)
    assert np.array_equal(g.bootstrap.theta_replicates, want.theta_replicates, equal_nan=True)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, in order, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS + ORDER:
        assert lib.vc_gene_joint_weighted(*jntw_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_joint_weighted(*jntw_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="weights"):
        gene_joint_weighted(np.ones((4, 2), np.float32), np.ones((4, 2), np.float32), Q.directions(np.arange(4.0)), np.ones(4), np.ones(3), 0.4)
    assert _WeightedProblem.__mro__[1].__name__ == "_Problem"
