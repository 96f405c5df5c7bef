"""GPU: the pointwise predictive density (velocycle_amd.predictive / vc_pointwise_density) against the float64 checker
(tests/pointwise_checker.py) on the fixtures written from the reference's own model (tests/golden/ref_pointwise_*.npz).
Bars: 4 x the worst error ratio the float32 reference itself shows over the fixtures, per quantity, in units of eps32 A (the checker's
forward rounding scale); no element, gene or cell is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pointwise_checker as PC
from tests.test_pointwise_cpu import CASES, bars, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GENE_KEYS = {"in_S": 0, "in_U": 0, "in_mu_nu": 0, "in_sd_nu": 0, "in_mu_gamma": 0, "in_sd_gamma": 0, "in_mu_beta": 0, "in_sd_beta": 0,
             "draw_ν": 1, "draw_Δν": 2, "draw_shape_inv": 1, "draw_logγg": 1, "draw_logβg": 1, "cond_ν": 0, "cond_shape_inv": 0}
CELL_KEYS = {"in_S": 1, "in_U": 1, "in_count_factor": 0, "in_Db": 1, "in_D": 1, "in_phixy_prior": 0, "draw_ϕxy": 1, "cond_ϕxy": 0}


def engine_of(z, **kw):
    from velocycle_amd.engine import HipEngine
    return HipEngine(H.spec_from_fixture(z), device=DEV, **kw)


def draws_of(z):
    return {k[len("draw_"):]: torch.tensor(v) for k, v in z.items() if k.startswith("draw_")}


def cut(z, Ng=None, Nc=None, D=None, cell_index=None):
    """The fixture's problem on genes arange(Ng) % Ng0, cells arange(Nc) % Nc0 (or `cell_index`), draws arange(D) % D0."""
    z = dict(z)
    Ng0, Nc0 = z["in_S"].shape
    gi = np.arange(Ng0 if Ng is None else Ng) % Ng0
    ci = (np.arange(Nc0 if Nc is None else Nc) % Nc0) if cell_index is None else np.asarray(cell_index)
    D0 = int(z["n_draws"])
    di = np.arange(D0 if D is None else D) % D0
    for k in list(z):
        if k in GENE_KEYS and np.ndim(z[k]) > GENE_KEYS[k]:
            z[k] = np.take(z[k], gi, axis=GENE_KEYS[k])
        if k in CELL_KEYS and np.ndim(z[k]) > CELL_KEYS[k]:
            z[k] = np.take(z[k], ci, axis=CELL_KEYS[k])
        if k.startswith("draw_") and z[k].shape[0] > 1:
            z[k] = np.take(z[k], di, axis=0)
    z["n_draws"] = np.int64(len(di))
    return z


def got_of(rec, dense=True):
    name = {"lppd": "lppd", "mean": "mean", "pwaic": "p_waic"}
    out = {}
    for m in rec.lppd_cell:
        out[m] = {q: {"gene": getattr(rec, name[q] + "_gene")[m], "cell": getattr(rec, name[q] + "_cell")[m],
                      "dense": rec.pointwise[m] if (dense and q == "lppd" and rec.pointwise is not None) else None} for q in PC.QUANT}
    return out


def assert_within_bars(tag, rec, z):
    e64 = PC.evaluate(z)
    r = PC.ratios(got_of(rec), e64)
    b = bars()
    print(f"{tag}: error ratios (eps32 A) " + ", ".join(f"{q} {r[q]:.3f} (bar {b[q]:.2f})" for q in PC.QUANT))
    for q in PC.QUANT:
        assert r[q] <= b[q], (tag, q, r[q], b[q])
    return r


def same_bits(a, b, cells_only=False):
    fields = ["lppd_cell", "mean_cell", "p_waic_cell"] + ([] if cells_only else ["lppd_gene", "mean_gene", "p_waic_gene"])
    for f in fields:
        for m in getattr(a, f):
            if not torch.equal(getattr(a, f)[m], getattr(b, f)[m]):
                return False
    if a.pointwise is not None and b.pointwise is not None:
        return all(torch.equal(a.pointwise[m], b.pointwise[m]) for m in a.pointwise)
    return True


@pytest.mark.parametrize("case", CASES)
def test_fixture_within_the_reference_s_bars(case):
    from velocycle_amd.predictive import pointwise_density
    z = load(case)
    eng = engine_of(z)
    rec = pointwise_density(eng, draws_of(z), return_pointwise=True)
    assert rec.n_draws == int(z["n_draws"])
    assert_within_bars(case, rec, z)
    for m in rec.lppd_gene:
        for f in ("lppd", "mean", "p_waic"):
            g, c = getattr(rec, f + "_gene")[m].sum().item(), getattr(rec, f + "_cell")[m].sum().item()
            assert abs(g - c) <= 1e-12 * max(abs(g), abs(c)), (case, m, f, g, c)
    eng.close()


@pytest.mark.parametrize("base,Nc,Ng,D", [("vel_mf_joint_nb", 1, 7, 2), ("vel_mf_joint_nb", 63, 1, 3), ("vel_mf_joint_nb", 65, 257, 2),
                                          ("vel_mf_joint_nb", 1000, 7, 50), ("phase_h2_poisson", 65, 257, 3), ("phase_nb", 1000, 1, 2),
                                          ("vel_mf_dnu2", 63, 7, 50)])
def test_ragged_shapes_against_the_checker(base, Nc, Ng, D):
    from velocycle_amd.predictive import pointwise_density
    z = cut(load(base), Ng=Ng, Nc=Nc, D=D)
    eng = engine_of(z)
    rec = pointwise_density(eng, draws_of(z), return_pointwise=True)
    assert rec.lppd_cell["S"].shape == (Nc,) and rec.lppd_gene["S"].shape == (Ng,) and rec.pointwise["S"].shape == (Ng, Nc)
    assert_within_bars(f"{base} {Nc} x {Ng} x {D}", rec, z)
    eng.close()


def test_storage_repeat_and_chunking_give_identical_bits():
    from velocycle_amd.predictive import pointwise_density
    from velocycle_amd.tuning import Tuning
    z = cut(load("vel_mf_joint_nb"), Nc=1000)
    dr = draws_of(z)
    e16, e32 = engine_of(z), engine_of(z, tuning=Tuning(count_storage="f32"))
    assert (e16.stats["count_storage"], e32.stats["count_storage"]) == ("u16", "f32")
    a = pointwise_density(e16, dr, return_pointwise=True)
    assert same_bits(a, pointwise_density(e32, dr, return_pointwise=True)), "uint16 and float32 count storage differ"
    assert same_bits(a, pointwise_density(e16, dr, return_pointwise=True)), "two calls differ"
    for chunk in (64, 1000, None):
        assert same_bits(a, pointwise_density(e16, dr, return_pointwise=True, chunk_cells=chunk)), f"chunk_cells={chunk} differs"
    e16.close(), e32.close()


def test_interleaved_batches_report_in_the_caller_s_order():
    from velocycle_amd.predictive import pointwise_density
    z0 = load("vel_mf_dnu2")
    Nc = z0["in_S"].shape[1]
    perm = np.random.default_rng(3).permutation(Nc)
    z = cut(z0, cell_index=perm)
    assert (np.diff(np.argmax(z["in_Db"], 0)) != 0).sum() > 10               # the batches are interleaved: the engine reorders the cells
    e0, e1 = engine_of(z0), engine_of(z)
    assert e1.stats["onehot_batches"] == 2
    a, b = pointwise_density(e0, draws_of(z0), return_pointwise=True), pointwise_density(e1, draws_of(z), return_pointwise=True)
    assert_within_bars("interleaved batches", b, z)
    for f in ("lppd_cell", "mean_cell", "p_waic_cell"):
        for m in ("S", "U"):
            assert torch.equal(getattr(a, f)[m][perm], getattr(b, f)[m]), (f, m)
    assert torch.equal(a.pointwise["U"][:, perm], b.pointwise["U"])
    for m in ("S", "U"):
        assert torch.allclose(a.lppd_gene[m], b.lppd_gene[m], rtol=1e-12, atol=0)
    e0.close(), e1.close()


def test_draw_invariant_S_is_evaluated_once():
    from velocycle_amd.predictive import pointwise_density
    z = load("vel_lrmn_cond")
    eng = engine_of(z)
    assert "vu_" in eng.stats["main_kernel"]                                # the tutorial conditioning
    full = {k: (v.expand((int(z["n_draws"]),) + tuple(v.shape[1:])).clone() if v.shape[0] == 1 else v) for k, v in draws_of(z).items()}
    for dr in (draws_of(z), full):                                           # given once, or repeated per draw as sample_posterior delivers them
        rec = pointwise_density(eng, dr)
        assert bool((rec.p_waic_gene["S"] == 0).all()) and bool((rec.p_waic_cell["S"] == 0).all())
        assert torch.equal(rec.lppd_gene["S"], rec.mean_gene["S"]) and torch.equal(rec.lppd_cell["S"], rec.mean_cell["S"])
        assert bool((rec.p_waic_cell["U"] > 0).all())
    eng.close()


def test_two_ranks_on_the_halves_of_a_problem():
    from velocycle_amd.engine import HipEngine, shard_bounds
    from velocycle_amd.predictive import merge_shards, pointwise_density
    z = load("vel_mf_joint_nb")
    spec, dr = H.spec_from_fixture(z), draws_of(z)
    one = HipEngine(spec, device=DEV)
    whole = pointwise_density(one, dr, return_pointwise=True)
    parts = []
    for r in range(2):
        c0, c1 = shard_bounds(spec.Nc, r, 2)
        e = HipEngine(spec, device=DEV, rank=r, world_size=2)
        parts.append(pointwise_density(e, {k: (v[:, c0:c1] if k == "ϕxy" else v) for k, v in dr.items()}, return_pointwise=True))
        e.close()
    both = merge_shards(parts)
    assert same_bits(whole, both, cells_only=True)
    for f in ("lppd_gene", "mean_gene", "p_waic_gene"):
        for m in ("S", "U"):
            assert torch.allclose(getattr(whole, f)[m], getattr(both, f)[m], rtol=1e-12, atol=1e-300), (f, m)
    one.close()


def test_end_to_end_prefers_the_right_model():
    """Tutorial flow at 2 x 1 500 cells x 200 genes of simulate_counts data, then: fit.predictive_density() is finite, and compare() of the
    fit against the same fit with nu cut down to its constant harmonic (a deliberately wrong model, explicit draws) prefers the right
    one by more than 5 standard errors."""
    from velocycle_amd import containers as Cn, preprocessing as P, pyro_compat as pyro
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.fit_models import PhaseFitModel, VelocityFitModel
    from velocycle_amd.optim import ClippedAdam
    from velocycle_amd.predictive import compare, pointwise_density
    from velocycle_amd.workloads import make_velocity_spec
    sp = make_velocity_spec(Nc=1500, Ng=200, n_conditions=2, Hw=0, seed=5)
    ad = AnnDataLite(sp.S.t().numpy(), sp.U.t().numpy())
    ad.obs["batch"] = [f"s{int(b)}" for b in sp.truth["batch"]]
    cyc = Cn.Cycle.from_array(sp.mu_nu.T.numpy(), sp.sd_nu.T.numpy(), list(ad.var.index))
    ph = Cn.Phases.from_array(sp.phixy_prior.T.numpy(), cell_names=list(ad.obs.index))
    Db = P.make_design_matrix(ad, ids="batch")
    n = 400
    opt = lambda: ClippedAdam({"lr": 0.03, "lrd": (0.005 / 0.03) ** (1 / n), "betas": (0.80, 0.99)})
    torch.manual_seed(3)
    pyro.clear_param_store()
    mp = P.preprocess_for_phase_estimation(ad, cyc, ph, Db, n_harmonics=1)
    pf = PhaseFitModel(mp, num_samples=20, n_per_bin=20)
    pf.fit(opt(), num_steps=n, verbose=False)
    keys = set(pf.posterior)
    rec_phase = pf.predictive_density(seed=1)
    assert set(pf.posterior) == keys and rec_phase.n_draws == 20 and np.isfinite(rec_phase.elpd_waic) and set(rec_phase.lppd_cell) == {"S"}
    cond = {"ϕxy": pf.phase_pyro.phi_xy_tensor.T, "ν": pf.cycle_pyro.means_tensor.T.unsqueeze(-2),
            "Δν": torch.tensor(pf.delta_nus), "shape_inv": torch.tensor(pf.disp_pyro).unsqueeze(-1)}
    spd = Cn.AngularSpeed.trivial_prior(condition_names=["s0", "s1"], harmonics=0)
    pyro.clear_param_store()
    mv = P.preprocess_for_velocity_estimation(ad, pf.cycle_pyro, pf.phase_pyro, spd, Db.float(), Db.float(), n_harmonics=1,
                                              count_factor=mp.count_factor, ω_n_harmonics=0, condition_on=cond)
    vf = VelocityFitModel(mv, condition_on=cond, num_samples=50, n_per_bin=50)
    vf.fit(opt(), num_steps=n, verbose=False)
    rec = vf.predictive_density(seed=2)
    assert rec.n_draws == 50 and set(rec.lppd_cell) == {"S", "U"} and rec.lppd_cell["U"].shape == (3000,)
    for f in ("lppd_gene", "lppd_cell", "mean_gene", "mean_cell", "p_waic_gene", "p_waic_cell"):
        assert all(bool(torch.isfinite(v).all()) for v in getattr(rec, f).values()), f
    assert np.isfinite(rec.waic) and rec.p_waic >= 0 and bool((rec.p_waic_cell["S"] == 0).all())
    eng = vf.engine
    draws = eng.sample_posterior(["ν", "Δν", "ϕxy", "shape_inv", "logγg", "logβg", "νω"], 50, seed=7)
    right = pointwise_density(eng, draws)
    wrong_draws = dict(draws)
    wrong_draws["ν"] = draws["ν"].clone()
    wrong_draws["ν"][:, :, 1:] = 0.0
    wrong = pointwise_density(eng, wrong_draws)
    d, se = compare(right, wrong)
    print(f"\n[end to end 3 000 x 200] elpd_waic right {right.elpd_waic:.1f}, constant-harmonic model {wrong.elpd_waic:.1f}; "
          f"paired difference {d:.1f} +- {se:.1f} ({d / se:.1f} standard errors)")
    assert d > 5 * se > 0


def _direct_call(eng, n_draws=4):
    one = C.c_void_p(64)                    # never dereferenced: the call is refused before anything is launched
    return eng.lib.vc_pointwise_density(eng._h, n_draws, one, 0, one, 0, one, one, one, 0, one, 0, one, 0, 0, 64, one, one, None, None)


def test_lognormal_and_run_time_sized_engines_are_refused_by_name():
    from velocycle_amd import _lib
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.predictive import pointwise_density
    from velocycle_amd.workloads import make_phase_spec
    for kw, word in ((dict(noisemodel="Lognormal"), "Lognormal"), (dict(H=4), "H = 4")):
        eng = HipEngine(make_phase_spec(Nc=200, Ng=20, **kw), device=DEV)
        eng.init_params()
        draws = eng.sample_posterior(["ν", "ϕxy"], 3, seed=1)
        with pytest.raises(NotImplementedError, match=word):
            pointwise_density(eng, draws)
        assert _direct_call(eng) == _lib.VC_ERR_UNSUPPORTED and word.encode() in eng.lib.vc_last_error(eng._h)
        eng.close()
