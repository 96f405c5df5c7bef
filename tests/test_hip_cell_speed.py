"""GPU: vc_cell_speed through `cell_angular_speed` and `grouped_angular_speed`, held to the reference and the bars of
tests/cell_speed_checker.py.  Every test prints the figures it asserts on."""
from dataclasses import fields

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import cell_speed_checker as Q
from tests.gene_kinetics_checker import directions
from tests.test_cell_speed_cpu import REFUSALS, csp_args
from velocycle_amd import _lib
from velocycle_amd import cell_speed as cs
from velocycle_amd.cell_speed import CellSpeedFit, GroupSpeedFit, cell_angular_speed, grouped_angular_speed, phase_bin_groups

pytestmark = pytest.mark.gpu

DOCUMENTED = (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED)
FLOATS = ("omega", "stds", "var", "loglik", "score", "fisher", "observed", "dec", "score_z", "rounding", "magnitude")


def inputs(p):
    disp = 1.0 / p["r"] if p["r"] is not None else 0.3
    return (p["U"].astype(np.float32), directions(p["phis"]), p["n"], p["nu"].T, p["x"], p["y"]), dict(noisemodel=p["noisemodel"], dispersion=disp)


def run(name, start=Q.START, **kw):
    args, nb = inputs(Q.cases()[name])
    return cell_angular_speed(*args, start, **nb, **kw)


def same_bits(a, b, cls=CellSpeedFit, rows=slice(None)):
    for f in fields(cls):
        x, y = getattr(a, f.name)[rows], getattr(b, f.name)[rows]
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), f.name


def assert_within_bars(name, fit, loglik_bar="loglik"):
    """The fit at the cells the reference CONVERGED on, and the score at the reference's own optimum (evaluate-only: the same point)."""
    bars, conv = Q.bars(), Q.check_case(name)
    sol = Q.solved(name)
    worst = dict(omega=0.0, var=0.0, fisher=0.0, observed=0.0, loglik=0.0, score=0.0)
    at = run(name, start=np.array([f64["om"] if f64["status"] == Q.CONVERGED else Q.START for f64, _ in sol]), evaluate_only=True)
    for c, f64, f32 in conv:
        assert fit.status[c] in Q.INTERIOR, (name, c, fit.status[c])
        worst["omega"] = max(worst["omega"], Q.omega_distance(fit.omega[c], f64))
        worst["var"] = max(worst["var"], Q.rel_distance(fit.var[c], 1.0 / f64["M"]))
        worst["fisher"] = max(worst["fisher"], Q.rel_distance(fit.fisher[c], f64["fisher"]))
        worst["observed"] = max(worst["observed"], Q.rel_distance(fit.observed[c], f64["observed"]))
        worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik[c], f64))
        worst["score"] = max(worst["score"], Q.score_distance(at.score[c], f64))
        assert fit.iterations[c] <= f32["iterations"] + 2, (name, c, fit.iterations[c], f32["iterations"])
        assert fit.n_clamped[c] == 0 and fit.stds[c] == 1.0 / np.sqrt(fit.fisher[c])
    for c, (f64, f32) in enumerate(sol):
        assert fit.status[c] in DOCUMENTED and (fit.status[c] in Q.INTERIOR or f32["status"] not in Q.INTERIOR), (name, c, fit.status[c])
    print(f"{name}: {len(conv)} of {len(sol)} cells; worst omega {worst['omega']:.3g} se (bar {bars['omega']:.3g}), var {worst['var']:.3g} "
          f"(bar {bars['var']:.3g}), fisher {worst['fisher']:.3g} (bar {bars['fisher']:.3g}), observed {worst['observed']:.3g} (bar "
          f"{bars['observed']:.3g}), objective {worst['loglik']:.3g} eps32 sum |log p| (bar {bars[loglik_bar]:.3g}), score "
          f"{worst['score']:.3g} noise units (bar {bars['score']:.3g}), steps {fit.iterations.max()}")
    assert all(worst[key] <= bars[key] for key in ("omega", "var", "fisher", "observed", "score")) and worst["loglik"] <= bars[loglik_bar]


@pytest.mark.parametrize("Nc,Ng,H,noise", [s[:4] for s in Q.SHAPES])
def test_shapes(Nc, Ng, H, noise):
    name = Q.shape_name(Nc, Ng, H, noise)
    fit = run(name)
    assert all(getattr(fit, f.name).shape == (Nc,) for f in fields(fit))
    assert fit.status.dtype == fit.iterations.dtype == fit.n_clamped.dtype == np.int32
    assert_within_bars(name, fit)


@pytest.mark.parametrize("name", Q.LARGE_CASES)
def test_large_counts(name):
    top = Q.cases()[name]["U"].max()
    assert top > 65535 if name == "large_f32" else 2e4 <= top <= 65535
    assert_within_bars(name, run(name), "loglik_large")
    if name == "large_u16":
        same_bits(run(name), run(name, storage="f32"))


def test_evaluate_only():
    """The objective, the score and n_clamped at five speeds per cell; the last one clamps genes: n_clamped is the count of a float64
    evaluation of the same float32 tables."""
    bars, worst, Nc = Q.bars(), dict(loglik=0.0, score=0.0), 65
    for i, om in enumerate(Q.EVALUATE_AT):
        fit = run(Q.EVALUATE_CASE, start=om, evaluate_only=True)
        assert all(np.isfinite(getattr(fit, f)).all() for f in FLOATS)
        assert (fit.status == Q.EVALUATED).all() and (fit.iterations == 0).all() and (fit.omega == om).all()
        assert np.array_equal(fit.score_z, fit.score / np.sqrt(fit.fisher))
        for c in range(Nc):
            ref, f32 = Q.evaluated()[(i, c)]
            worst["loglik"] = max(worst["loglik"], Q.loglik_distance(fit.loglik[c], ref))
            worst["score"] = max(worst["score"], Q.score_distance(fit.score[c], ref))
            assert fit.n_clamped[c] == f32["n_clamped"], (i, c)
        print(f"omega {om}: clamped genes {fit.n_clamped.sum()}, worst so far {worst}")
    assert fit.n_clamped.sum() > 0
    print(f"evaluate-only: objective {worst['loglik']:.3g} (bar {bars['ev_loglik']:.3g}), score {worst['score']:.3g} (bar {bars['ev_score']:.3g})")
    assert worst["loglik"] <= bars["ev_loglik"] and worst["score"] <= bars["ev_score"]


def test_kink_case_keeps_what_holds_there():
    """63 x 5, NB, defaults: cells kink and run to |omega| of 3.  Finite outputs, a documented status, f no lower than at the start, and
    n_clamped the float64 count at the kernel's own point (no gene within 1e-9 of the kink there)."""
    name = Q.KINK_CASE
    fit = run(name, max_iter=60)
    Nc = len(fit.omega)
    for c in range(Nc):
        at, at0 = Q.at32(name, [c], fit.omega[c]), Q.at32(name, [c], Q.START)
        ref, ref0 = Q.at64(name, [c], fit.omega[c]), Q.at64(name, [c], Q.START)
        assert fit.status[c] in DOCUMENTED and fit.n_clamped[c] == at["n_clamped"], (c, fit.status[c], fit.n_clamped[c], at["n_clamped"])
        assert ref["f"] >= ref0["f"] - 8 * Q.EPS32 * max(at["A"], at0["A"]), (c, ref["f"], ref0["f"])
    print(f"{name}: status counts {np.bincount(fit.status, minlength=6)}, omega {fit.omega.min():.3g} .. {fit.omega.max():.3g}, steps "
          f"<= {fit.iterations.max()}, clamped genes {fit.n_clamped.sum()}")
    assert all(np.isfinite(getattr(fit, f)).all() for f in FLOATS)
    assert np.abs(fit.omega).max() > 1.5


def test_cells_without_data_touch_no_neighbour():
    name = "shape_257_3_1_Poisson"
    (U, xy, n, means, lg, lb), nb = inputs(Q.cases()[name])
    ref = cell_angular_speed(U, xy, n, means, lg, lb, Q.START, **nb)
    empty = U.copy()
    empty[[0, 64, 130]] = 0
    start = np.full(257, Q.START)
    start[[5, 200]] = [np.nan, np.inf]
    cases = [(cell_angular_speed(empty, xy, n, means, lg, lb, Q.START, **nb), [0, 64, 130], ref),
             (cell_angular_speed(U, xy, n, means, lg, lb, start, **nb), [5, 200], ref)]
    prior = np.stack([np.zeros(257), np.full(257, 3.0)], 1)
    with_prior = cell_angular_speed(U, xy, n, means, lg, lb, Q.START, prior=prior, **nb)
    bad = prior.copy()
    bad[[7, 66, 100, 256]] = [[0.0, 0.0], [np.nan, 1.0], [0.0, np.inf], [0.0, -1.0]]
    cases.append((cell_angular_speed(U, xy, n, means, lg, lb, Q.START, prior=bad, **nb), [7, 66, 100, 256], with_prior))
    for got, gone, want in cases:
        keep = np.setdiff1d(np.arange(257), gone)
        assert (got.status[gone] == Q.NO_DATA).all() and (got.iterations[gone] == 0).all() and (got.n_clamped[gone] == 0).all()
        assert all(np.isnan(getattr(got, f)[gone]).all() for f in FLOATS)
        same_bits(got, want, rows=keep)                                    # the neighbours: bit for bit
        assert (got.status[keep] != Q.NO_DATA).all()
    one = run(name, max_iter=1)
    print("max_iter = 1:", np.bincount(one.status, minlength=6), one.iterations.max())
    moved = one.status == Q.MAX_ITER
    assert moved.sum() >= 200 and (one.iterations[moved] == 1).all() and (one.iterations <= 1).all()


def test_bit_equal_across_chunks_storage_input_stride_and_repetition():
    for name in ("shape_257_3_1_Poisson", "shape_64_65_2_NegativeBinomial"):
        (U, xy, n, means, lg, lb), nb = inputs(Q.cases()[name])
        ref = cell_angular_speed(U, xy, n, means, lg, lb, Q.START, **nb)
        for extra in (dict(), dict(chunk_cells=1), dict(chunk_cells=64), dict(chunk_cells=65), dict(chunk_cells=100), dict(storage="f32"),
                      dict(storage="u16")):
            same_bits(ref, cell_angular_speed(U, xy, n, means, lg, lb, Q.START, **nb, **extra))
        same_bits(ref, cell_angular_speed(sp.csr_matrix(U), xy, n, means, lg, lb, Q.START, **nb, chunk_cells=70))
        same_bits(ref, cell_angular_speed(torch.as_tensor(U).cuda(), xy, n, means, lg, lb, Q.START, **nb))
        # gene_stride > Nc: rows of the block further apart, with counts between them that belong to no cell
        keep, basis, logm, nu, xk, r = cs.check_arguments(U, xy, n, means, lg, lb, **nb)
        outs = []
        for pad in (0, 3):
            prob = cs._Problem(U, basis, logm, nu, xk, r, nb["noisemodel"], None, 100, "auto", stride_pad=pad)
            assert all(int(kblk.shape[1]) == c1 - c0 + pad for c0, c1, kblk, _, _ in prob.chunks)
            outs.append({k: v.cpu().numpy() for k, v in prob.run(np.full(U.shape[0], Q.START), None, 1e-10, 25).items()})
        assert all(np.array_equal(outs[0][k], outs[1][k], equal_nan=True) for k in outs[0])
        assert np.array_equal(outs[0]["omega"], ref.omega) and np.array_equal(outs[0]["sums"][:, 1], ref.score)
    # a mask of genes is the fit of those genes, and a prior pulls towards its mean
    name = "shape_65_64_1_Poisson"
    (U, xy, n, means, lg, lb), nb = inputs(Q.cases()[name])
    mask = np.arange(64) % 3 != 0
    same_bits(cell_angular_speed(U, xy, n, means, lg, lb, Q.START, genes=mask, **nb),
              cell_angular_speed(U[:, mask], xy, n, means[:, mask], lg[mask], lb[mask], Q.START, **nb))
    free, tight = run(name), run(name, prior=(0.0, 0.05))
    assert (np.abs(tight.omega) < np.abs(free.omega)).mean() > 0.9 and (tight.stds < free.stds).all()


@pytest.mark.parametrize("name", Q.GROUP_CASES)
def test_grouped_fit(name):
    p = Q.cases()[name]
    args, nb = inputs(p)
    groups, centres = phase_bin_groups(args[1], Q.GROUPS[name], p["D"])
    ref = Q.group_solved(name)
    G = len(ref)
    fit = grouped_angular_speed(*args, groups, Q.START, **nb, n_groups=G + 1)      # the last group has no cell
    bars, worst = Q.bars(), dict(group=0.0, group_std=0.0, truth=0.0)
    for g, (f64, f32, rows) in enumerate(ref):
        truth = Q.true_speed(p)[rows].mean()
        d = dict(group=Q.omega_distance(fit.omega[g], f64), group_std=Q.rel_distance(fit.stds[g], f64["se"]),
                 truth=abs(fit.omega[g] - truth) / fit.stds[g])
        print(f"{name} group {g}: omega {fit.omega[g]:.5f} +- {fit.stds[g]:.4f}, {d['group']:.3g} se from the reference, truth "
              f"{truth:.4f} ({d['truth']:.2f} se), {fit.rounds[g]} steps (restatement {f32['iterations']}), status {fit.status[g]}")
        worst = {k: max(worst[k], d[k]) for k in worst}
        assert fit.status[g] in Q.INTERIOR and fit.rounds[g] <= f32["iterations"] + 2 and fit.n_cells[g] == len(rows) and fit.n_clamped[g] == 0
        assert Q.loglik_distance(fit.loglik[g], f64) <= bars["loglik"] and Q.rel_distance(fit.fisher[g], f64["fisher"] ) <= bars["fisher"]
    print(f"{name}: worst {worst['group']:.3g} se (bar {bars['group']:.3g}), stds off by {worst['group_std']:.3g} (bar {bars['group_std']:.3g})")
    assert worst["group"] <= bars["group"] and worst["group_std"] <= bars["group_std"] and worst["truth"] <= 4.0
    assert fit.status[G] == Q.NO_DATA and fit.n_cells[G] == 0 and fit.rounds[G] == 0 and fit.n_clamped[G] == 0
    assert all(np.isnan(getattr(fit, f)[G]) for f in ("omega", "stds", "var", "loglik", "score", "fisher", "observed", "dec"))
    for extra in (dict(), dict(chunk_cells=64), dict(chunk_cells=333, storage="f32")):
        same_bits(fit, grouped_angular_speed(*args, groups, Q.START, **nb, n_groups=G + 1, **extra), GroupSpeedFit)


def test_groups_of_one_cell_are_the_per_cell_fit():
    """groups = arange(Nc) under the groups' default prior against `cell_angular_speed` under the same prior: the same sums, the rules
    once on the host and once in the kernel."""
    name = "shape_65_64_1_Poisson"
    args, nb = inputs(Q.cases()[name])
    Nc = 65
    cells = cell_angular_speed(*args, Q.START, **nb, prior=Q.GROUP_PRIOR)
    grouped = grouped_angular_speed(*args, np.arange(Nc), Q.START, **nb)
    d = np.abs(grouped.omega - cells.omega) / np.sqrt(cells.var)
    sol = Q.solved(name, Q.GROUP_PRIOR)
    dref = max(Q.omega_distance(cells.omega[c], sol[c][0]) for c in range(Nc))
    print(f"grouped against per-cell: {d.max():.3g} se, per-cell against the reference {dref:.3g} se (bar {Q.bars()['omega']:.3g}); steps "
          f"{grouped.rounds.max()} and {cells.iterations.max()}")
    assert d.max() <= Q.bars()["omega"] and dref <= Q.bars()["omega"]
    assert np.array_equal(grouped.status, cells.status) and np.abs(grouped.rounds - cells.iterations).max() <= 1
    assert np.abs(grouped.stds / cells.stds - 1).max() <= Q.bars()["fisher"] and (grouped.n_cells == 1).all()


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS:
        assert lib.vc_cell_speed(*csp_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_cell_speed(*csp_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
