"""GPU: the count-histogram paths of the negative binomial held to the float64 oracle at large counts.

The lgamma / digamma terms of the negative binomial never go through K_main: they come from per-gene count histograms, evaluated
as dense tail-count tables (integer counts < 2048: vc_build_dense_hist, vc_hist_dense_block, vc_hist_dense16_issue / _finish and
their quarter-block form) or as (value, multiplicity) lists with the Stirling difference vc_lgamma_digamma_diff (any count >= 2048
or not an integer; the phase model's and the sharded default).  The data of tests/helpers.py: boundary_spec put genes at the
level limits of those evaluators (largest count of a quarter 255, 256, 257, 639, 640, 641, 2047, 700 next to an all-zero
quarter, an all-zero block) and one extra count that forces the lists (2048, 65535) and float32 storage (65536, 7.5, 1e5 + 0.5).

Bars: the loss within 1e-5 of the float64 oracle and every gradient block within the bars of assert_step_matches_oracle; in
addition every gene's shape_inv_locs gradient within GENE_RTOL of that gene's sum of absolute terms (a block max-norm cannot see one
missing count level; tests/test_count_extremes_cpu.py proves that this bar can)."""
import numpy as np
import pytest
import torch

from oracle import velocycle_oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu
GENE_RTOL = H.GENE_RTOL     # the per-gene bar of the shape_inv_locs gradient (its sensitivity: tests/test_count_extremes_cpu.py)
STIRLING_RTOL = 1e-5        # the same on the Stirling path alone: ~1e-6 relative error per value (vc_common.h), x 10


def _cov(spec, seed=0):
    if not (spec.kind == "velocity" and spec.guide == "lrmn"):
        return None
    g = torch.Generator().manual_seed(seed)
    M = spec.Ng + spec.Nx * spec.Nhw
    return torch.normal(torch.zeros((M, spec.rho_rank)), torch.ones((M, spec.rho_rank)) * 0.02, generator=g)


def _gene_check(eng, spec, eps, g64, rtol):
    """Every gene's shape_inv_locs gradient against the float64 oracle, relative to the gene's sum of absolute terms."""
    if spec.noisemodel != "NegativeBinomial" or "shape_inv" in spec.condition_on or spec.guide != "meanfield":
        return 0.0                      # (where its sensitivity holds: tests/test_count_extremes_cpu.py)
    par = {n: v.detach().cpu() for n, v in eng.named().items()}
    _, scale, _ = H.nb_shape_inv_terms(spec, par, eps)
    got = eng.named(eng.grad)["shape_inv_locs"].cpu().double().numpy()
    want = g64["shape_inv_locs"].numpy()
    ratio = np.abs(got - want) / scale
    worst = int(ratio.argmax())
    assert ratio.max() <= rtol, (worst, got[worst], want[worst], scale[worst], ratio.max())
    return float(ratio.max())


def _step(spec, tuning=None, seed=1, expect_storage=None, expect_split=None, params=None, gene_rtol=GENE_RTOL, loss_rtol=1e-5):
    """One ELBO + gradient evaluation on explicit eps against the float64 oracle; returns the engine's stats."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.rng import draw_eps
    eng = HipEngine(spec, tuning=tuning)
    try:
        st = dict(eng.stats)
        if expect_storage is not None:
            assert st["count_storage"] == expect_storage, st
        if expect_split is not None:
            assert st["hist_split"] == expect_split, st
        eng.init_params(_cov(spec))
        if params:
            eng.set_params(params)
        eps = draw_eps(spec, torch.Generator().manual_seed(seed))
        eng.elbo_grad(eps=eng.pack_eps(eps))
        _, g64 = H.assert_step_matches_oracle(eng, spec, eps, loss_rtol=loss_rtol)
        worst = _gene_check(eng, spec, eps, g64, gene_rtol)
        print(f"[count extremes] {spec.kind}/{spec.guide}/{spec.noisemodel} {st['main_kernel']} storage {st['count_storage']} "
              f"hist_split {st['hist_split']}: shape_inv_locs per-gene error {worst:.2e} of the gene's absolute terms")
        assert eng.status()[0]
        return st
    finally:
        eng.close()


def _T(**kw):
    from velocycle_amd.tuning import Tuning
    return Tuning(**kw)


# (blocks past 256 levels: 0 (2047), 1 (700), 3 (639) -- per matrix; hist_split counts (matrix, block) pairs)
SPLIT = {"phase": 3, "velocity": 6}


@pytest.mark.parametrize("storage", ["u16", "f32"])
@pytest.mark.parametrize("form", ["lists", "dense"])
def test_phase_nb(form, storage):
    """Phase model: the lists are its default (hist_split 0); dense forced (hist_dense="dense": every count an integer < 2048)."""
    spec = H.boundary_spec("phase")
    tun = _T(hist_dense="dense" if form == "dense" else None, count_storage="f32" if storage == "f32" else None)
    _step(spec, tun, expect_storage=storage, expect_split=SPLIT["phase"] if form == "dense" else 0)


@pytest.mark.parametrize("storage", ["u16", "f32"])
@pytest.mark.parametrize("form", ["dense", "lists"])
def test_vjoint_nb_meanfield(form, storage):
    """V-joint mean-field: dense tables are the single-rank default; the lists forced."""
    spec = H.boundary_spec("vjoint")
    tun = _T(hist_dense="lists" if form == "lists" else None, count_storage="f32" if storage == "f32" else None)
    _step(spec, tun, expect_storage=storage, expect_split=SPLIT["velocity"] if form == "dense" else 0)


@pytest.mark.parametrize("overflow", [2048.0, 65535.0, 65536.0, 7.5, 100000.5])
def test_vjoint_nb_overflow_count_forces_lists(overflow):
    """One count >= 2048 or not an integer: the lists for the whole matrix (no dense table: hist_split 0), and float32 storage for
    a count > 65535 or a non-integer one (OVERFLOW_VARIANTS)."""
    form, storage = H.OVERFLOW_VARIANTS[overflow]
    spec = H.boundary_spec("vjoint", overflow=overflow)
    _step(spec, None, expect_storage=storage, expect_split=0)


def test_vjoint_nb_lrmn():
    _step(H.boundary_spec("vjoint_lrmn"), None)


@pytest.mark.parametrize("storage", ["u16", "f32"])
def test_vcond_tutorial_stage(storage):
    """The conditioned stage (shape_inv conditioned): the histogram sums are a constant of the loss, formed once in vc_finalize."""
    spec = H.boundary_spec("vcond")
    _step(spec, _T(count_storage="f32" if storage == "f32" else None), expect_storage=storage)


@pytest.mark.parametrize("kind,noise,storage,overflow", [("vjoint", "Poisson", "u16", None), ("vjoint", "Poisson", "f32", None),
                                                         ("phase", "Poisson", "u16", None), ("vjoint", "Poisson", "f32", 65536.0),
                                                         ("vjoint", "Lognormal", "f32", None), ("phase", "Lognormal", "f32", 100000.5)])
def test_poisson_and_lognormal_stream_the_same_counts(kind, noise, storage, overflow):
    spec = H.boundary_spec(kind, noisemodel=noise, overflow=overflow)
    forced = storage == "f32" and noise == "Poisson" and overflow is None
    _step(spec, _T(count_storage="f32") if forced else None, expect_storage=storage)


# ---------------------------------------------------------------------------------------------------------------------
# The Stirling path on its own: r = 1 / shape_inv over 1e-4 .. 1e4, counts k from 1 to 1e6 and non-integers
# ---------------------------------------------------------------------------------------------------------------------
STIRLING_K = (1.0, 2.0, 7.0, 8.0, 100.0, 2047.0, 2048.0, 65535.0, 65536.0, 1e6, 0.5, 7.5, 100000.5)
STIRLING_R = tuple(10.0 ** e for e in (-4, -3, -2, -1, 0, 1, 2, 3, 4))


def _stirling_spec():
    """Phase NB, phi_xy and nu conditioned: gene (i, j) has r = STIRLING_R[i] (set through shape_inv_locs, a point parameter) and
    count STIRLING_K[j] on 5 of its 24 cells (zero elsewhere); its nu sits at the log of the gene's mean count."""
    from velocycle_amd.workloads import make_phase_spec
    nr, nk, Nc = len(STIRLING_R), len(STIRLING_K), 24
    spec = make_phase_spec(Nc, nr * nk, seed=4)
    S = torch.zeros(nr * nk, Nc)
    for i in range(nr):
        for j, k in enumerate(STIRLING_K):
            S[i * nk + j, j % 4: j % 4 + 5] = k
    spec.S = S
    mu = spec.mu_nu.clone()
    mu[:, 0] = torch.log(S.mean(1))
    mu[:, 1:] = 0.0
    spec.mu_nu = mu
    spec.condition_on = {"ϕxy": torch.stack([torch.cos(torch.arange(Nc) * 0.3), torch.sin(torch.arange(Nc) * 0.3)], 1), "ν": mu.clone()}
    r = torch.tensor([STIRLING_R[g // nk] for g in range(nr * nk)], dtype=torch.float64)
    return spec, {"shape_inv_locs": torch.log(1.0 / r).float()}


def test_stirling_difference_against_float64_lgamma_digamma():
    """Every gene's shape_inv_locs gradient within STIRLING_RTOL of its absolute terms.  The loss: within 1e-5 of the float64 loss
    plus 1e-7 of the absolute sum T of its histogram terms n (lgamma(r + k) - lgamma(r)).  At k = 1e6 those terms are 1.4e7 per
    cell, and the loss (2.2e6) is what is left of T = 6.5e8 after they cancel against the k log(...) terms of K_main: one float32
    rounding of the terms is 3e-5 of the loss.  Measured on an MI355X: 2.1e-5 of the loss = 7e-8 of T (the oracle's own float32 run:
    4.2e-6); a float32 model of vc_lgamma_digamma_diff is within 1.4e-7 of float64 at every (r, k) of the grid."""
    from scipy.special import gammaln
    from velocycle_amd.rng import draw_eps
    spec, par = _stirling_spec()
    r = (1.0 / torch.exp(par["shape_inv_locs"])).double().numpy()
    S = spec.S.double().numpy()
    T = float(np.abs(np.where(S > 0, gammaln(r[:, None] + S) - gammaln(r[:, None]), 0.0)).sum())
    p64 = H.problem_from_spec(spec, torch.float64)
    eng_par = orc.init_params(p64)
    eng_par["shape_inv_locs"] = par["shape_inv_locs"].double()
    eps = draw_eps(spec, torch.Generator().manual_seed(1))
    l64, _, _, _ = orc.loss_and_grads(p64, {k: v.float().double() for k, v in eng_par.items()},
                                      {k: v.double() for k, v in eps.items() if not k.startswith("_")})
    _step(spec, _T(hist_dense="lists"), seed=1, expect_storage="f32", expect_split=0, params=par, gene_rtol=STIRLING_RTOL,
          loss_rtol=1e-5 + 1e-7 * T / abs(l64))


# ---------------------------------------------------------------------------------------------------------------------
# The fused and sharded steps on the same data
# ---------------------------------------------------------------------------------------------------------------------
def _stats(spec, tuning=None, **kw):
    from velocycle_amd.engine import HipEngine
    e = HipEngine(spec, tuning=tuning, **kw)
    st = dict(e.stats)
    e.close()
    return st


@pytest.mark.parametrize("tail2", [True, False])
def test_fused_steps_dense_tables(tail2):
    """The benchmarked fused step (two launches by default, three with tail2=False) on dense tables: the two-launch tail gives the
    blocks past 256 levels quarter blocks of their own (hist_split), among them a block past 640 levels next to an empty quarter."""
    from tests.test_hip_fused_oracle import _fused_vs_oracle
    spec = H.boundary_spec("vjoint")
    tun = _T(hist_dense="dense", tail2=tail2)
    st = _stats(spec, tun)
    assert st["launches_per_step"] == (2 if tail2 else 3) and st["hist_split"] == SPLIT["velocity"], st
    _fused_vs_oracle(spec, n=8, seed=11, tuning=tun)


def test_fused_step_lists_through_an_overflow_count():
    from tests.test_hip_fused_oracle import _fused_vs_oracle
    spec = H.boundary_spec("vjoint", overflow=65536.0)
    st = _stats(spec)
    assert st["hist_split"] == 0 and st["count_storage"] == "f32", st
    _fused_vs_oracle(spec, n=8, seed=12)


def test_particle_step_k3_quarter_blocks():
    """K = 3 particles (K_pre's quarter blocks on dense tables) against orc.fit(num_particles=3) on the same Philox draws."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    spec = H.boundary_spec("vjoint")
    opt = {"lr": 0.03, "lrd": 0.99, "betas": (0.8, 0.99)}
    K, n, seed = 3, 6, 99
    eng = HipEngine(spec, tuning=_T(hist_dense="dense"))
    assert eng.stats["hist_split"] == SPLIT["velocity"]
    run = SVIRunner(eng, opt, mode="perf", seed=seed, num_particles=K)
    flat0 = eng.params.detach().clone()
    par0 = {k: v.detach().cpu().clone() for k, v in eng.named().items()}
    run.run_perf(n)
    losses = np.array(run.perf_losses())
    eps = H.philox_eps_list(spec, flat0, seed, n * K)
    p64 = H.problem_from_spec(spec, torch.float64)
    l64, par64 = orc.fit(p64, opt, n, eps_list=eps, params={k: v.double() for k, v in par0.items()}, num_particles=K)
    assert np.allclose(losses, l64, rtol=2e-5), np.abs(losses / np.array(l64) - 1).max()
    for k, v in eng.named().items():
        want, got = par64[k].numpy(), v.cpu().numpy().astype(np.float64)
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=2e-3, atol=2e-3), (k, np.abs(got[fin] - want[fin]).max())
    eng.close()


@pytest.mark.parametrize("overflow,form", [(None, "dense"), (None, None), (70000.0, None)])
def test_sharded_sequence_with_unequal_rank_tables(overflow, form):
    """World = 2, in-process ranks (K_main -> phase A -> exchange -> phase B): the boundary genes' top counts sit in rank 0's cells
    only, so rank 0's tables go past 256 / 640 levels where rank 1's stay below 200; with `overflow` rank 1 alone holds a count of
    70 000 (float32 storage there, uint16 on rank 0).  Lists are the sharded default; dense tables forced once.  Replayed step by step by the float64 oracle on the Philox draws it used."""
    from velocycle_amd.engine import HipEngine
    from tests.test_hip_sharded_step import OPT as SOPT, _run_sharded
    spec = H.boundary_spec("vjoint", overflow=overflow)
    world, n, seed = 2, 6, 0
    if overflow is not None:
        st = [_stats(spec, rank=r, world_size=world)["count_storage"] for r in range(world)]
        assert st == ["u16", "f32"], st
    tun = _T(hist_dense=form) if form else None
    if form == "dense":
        st = [_stats(spec, tun, rank=r, world_size=world) for r in range(world)]
        assert st[0]["hist_split"] == SPLIT["velocity"] and st[1]["hist_split"] == 0, st
    ranks = _run_sharded(spec, world, n, seed, tun)
    losses = ranks[0].ring[:n].cpu().numpy()
    got = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in ranks[0].e.named().items()}
    got["ϕxy_locs"] = torch.cat([r.e.view(r.e.params, "ϕxy_locs").detach().cpu() for r in ranks]).numpy().astype(np.float64)
    for r in ranks:
        assert r.e.status() == (True, -1, 0)
        r.e.close()
    e0 = HipEngine(spec)
    e0.init_params(None)
    par0 = {k: v.detach().cpu().clone() for k, v in e0.named().items()}
    flat0 = e0.params.detach().clone()
    e0.close()
    opt = {"lr": SOPT["lr"], "lrd": SOPT["lrd"], "betas": (SOPT["b1"], SOPT["b2"])}
    eps = H.philox_eps_list(spec, flat0, seed, n)
    l64, par64 = H.oracle_replay(spec, opt, par0, eps, torch.float64)
    l32, par32 = H.oracle_replay(spec, opt, par0, eps, torch.float32)
    l64, l32 = np.array(l64), np.array(l32)
    rel_hip, rel_32 = np.abs(losses - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
    assert rel_hip[:5].max() <= 1e-5, rel_hip[:5]
    assert (rel_hip <= np.maximum(1e-5, 4 * np.maximum.accumulate(rel_32))).all(), (rel_hip.max(), rel_32.max())
    H.assert_params_track_oracle(got, {k: v.numpy() for k, v in par64.items()}, {k: v.double().numpy() for k, v in par32.items()},
                                 report=f"sharded world=2, boundary counts, overflow {overflow}")
