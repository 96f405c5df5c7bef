"""GPU: phase-marginal scoring (velocycle_amd.predictive.phase_marginal / vc_phase_marginal) against the float64 checker
(tests/phase_marginal_checker.py) on the fixtures written from the reference's own model (tests/golden/ref_pointwise_*.npz).
Bars: 4 x the worst error ratio the checker's float32 restatement shows over the fixtures, per quantity, in the checker's units
(tests/test_phase_marginal_cpu.py::bars); no cell, bin or draw is left out of any comparison."""
import math

import numpy as np
import pytest
import torch

from tests import mle_checker as LC
from tests import phase_marginal_checker as MC
from tests import test_cycle_mle_cpu as LF
from tests.test_hip_pointwise import cut, draws_of, engine_of
from tests.test_phase_marginal_cpu import B_FIXTURES, CAL_BINS, CALIBRATION, Z_BAR, bars, checked, simulated
from tests.test_pointwise_cpu import CASES, load

pytestmark = pytest.mark.gpu
EPS32 = MC.EPS32


def got_of(rec):
    return {"evidence": rec.log_evidence, "post": rec.posterior, "per_draw": rec.per_draw}


def assert_sound(tag, rec):
    assert bool(torch.isfinite(rec.log_evidence).all()) and bool(torch.isfinite(rec.posterior).all()), tag
    assert rec.per_draw is None or bool(torch.isfinite(rec.per_draw).all()), tag
    assert bool((rec.posterior >= 0).all()), tag
    dev = float((rec.posterior.double().sum(1) - 1.0).abs().max())
    assert dev <= 64 * EPS32, (tag, dev)


def assert_within_bars(tag, rec, e64):
    assert_sound(tag, rec)
    r = MC.ratios(got_of(rec), e64)
    b = bars()
    print(f"{tag}: error ratios " + ", ".join(f"{q} {r[q]:.4f} (bar {b[q]:.2f})" for q in r))
    for q in r:
        assert r[q] <= b[q], (tag, q, r[q], b[q])
    return r


def same_bits(a, b):
    ok = torch.equal(a.log_evidence, b.log_evidence) and torch.equal(a.posterior, b.posterior)
    if a.per_draw is not None and b.per_draw is not None:
        ok = ok and torch.equal(a.per_draw, b.per_draw)
    return ok


@pytest.mark.parametrize("case", CASES)
def test_fixture_within_the_bars(case):
    from velocycle_amd.predictive import phase_marginal
    z, e64 = checked(case)
    eng = engine_of(z)
    dr = draws_of(z)
    rec = phase_marginal(eng, dr, bins=B_FIXTURES, phase_prior="flat", return_per_draw=True)
    Nc = z["in_S"].shape[1]
    assert rec.n_draws == int(z["n_draws"]) and rec.posterior.shape == (Nc, B_FIXTURES) and rec.per_draw.shape == (rec.n_draws, Nc)
    assert rec.log_evidence.dtype == torch.float64 and rec.posterior.dtype == torch.float32 and rec.per_draw.dtype == torch.float64
    assert_within_bars(case, rec, e64)
    # ϕxy is ignored when present and not required
    assert same_bits(rec, phase_marginal(eng, {k: v for k, v in dr.items() if k != "ϕxy"}, bins=B_FIXTURES, phase_prior="flat", return_per_draw=True))
    assert rec.elpd == pytest.approx(float(e64["evidence"].sum()), rel=1e-6)
    eng.close()


@pytest.mark.parametrize("base,Nc,Ng,D,B", [("vel_mf_joint_nb", 1, 7, 1, 2), ("vel_mf_joint_nb", 63, 1, 3, 33), ("vel_mf_joint_nb", 65, 257, 2, 64),
                                            ("phase_h2_poisson", 1, 7, 2, 4096), ("phase_nb", 1000, 7, 50, 32), ("vel_mf_dnu2", 63, 7, 8, 64)])
def test_ragged_shapes_against_the_checker(base, Nc, Ng, D, B):
    from velocycle_amd.predictive import phase_marginal
    z = cut(load(base), Ng=Ng, Nc=Nc, D=D)
    eng = engine_of(z)
    rec = phase_marginal(eng, draws_of(z), bins=B, phase_prior="flat", return_per_draw=True)
    assert rec.log_evidence.shape == (Nc,) and rec.posterior.shape == (Nc, B) and rec.per_draw.shape == (D, Nc) and rec.phis.shape == (B,)
    assert_within_bars(f"{base} {Nc} x {Ng} x {D} x {B}", rec, MC.evaluate(z, B))
    eng.close()


def test_chunking_storage_and_repetition_give_identical_bits():
    from velocycle_amd.predictive import phase_marginal
    from velocycle_amd.tuning import Tuning
    z = cut(load("vel_mf_joint_nb"), Nc=200, Ng=30, D=3)
    dr = draws_of(z)
    e16, e32 = engine_of(z), engine_of(z, tuning=Tuning(count_storage="f32"))
    assert (e16.stats["count_storage"], e32.stats["count_storage"]) == ("u16", "f32")
    kw = dict(bins=24, return_per_draw=True)
    a = phase_marginal(e16, dr, **kw)
    assert same_bits(a, phase_marginal(e32, dr, **kw)), "uint16 and float32 count storage differ"
    assert same_bits(a, phase_marginal(e16, dr, **kw)), "two calls differ"
    for chunk in (64, 128, 70):
        assert same_bits(a, phase_marginal(e16, dr, chunk_cells=chunk, **kw)), f"chunk_cells={chunk} differs"
    e16.close(), e32.close()


def test_interleaved_batches_report_in_the_caller_s_order():
    from velocycle_amd.predictive import phase_marginal
    z0 = cut(load("vel_mf_dnu2"), Ng=20)
    Nc = z0["in_S"].shape[1]
    perm = np.random.default_rng(3).permutation(Nc)
    z = cut(z0, cell_index=perm)
    assert (np.diff(np.argmax(z["in_Db"], 0)) != 0).sum() > 10               # the batches are interleaved: the engine reorders the cells
    e0, e1 = engine_of(z0), engine_of(z)
    assert e1.stats["onehot_batches"] == 2
    kw = dict(bins=16, return_per_draw=True)                                 # the default prior: the model's, a row per cell
    a, b = phase_marginal(e0, draws_of(z0), **kw), phase_marginal(e1, draws_of(z), **kw)
    assert torch.equal(a.log_evidence[perm], b.log_evidence) and torch.equal(a.posterior[perm], b.posterior)
    assert torch.equal(a.per_draw[:, perm], b.per_draw)
    e0.close(), e1.close()


def test_sites_given_once_or_in_equal_copies_give_identical_bits():
    """vel_lrmn_cond: nu, ϕxy and shape_inv are the same in every draw (the tutorial's conditioning) -- the spliced sums are formed once
    per (cell, bin).  The sites given once, or repeated per draw as sample_posterior delivers them: the same bits, within the bars."""
    from velocycle_amd.predictive import phase_marginal
    z = cut(load("vel_lrmn_cond"), Ng=40, Nc=130)
    eng = engine_of(z)
    once = draws_of(z)
    D = int(z["n_draws"])
    assert once["ν"].shape[0] == 1 and once["logγg"].shape[0] == D
    full = {k: (v.expand((D,) + tuple(v.shape[1:])).clone() if v.shape[0] == 1 else v) for k, v in once.items()}
    a = phase_marginal(eng, once, bins=20, phase_prior="flat", return_per_draw=True)
    assert same_bits(a, phase_marginal(eng, full, bins=20, phase_prior="flat", return_per_draw=True))
    assert_within_bars("vel_lrmn_cond, S formed once", a, MC.evaluate(z, 20))
    # the phase model with every site equal: every draw has the evidence of the first
    zp = cut(load("phase_nb"), Ng=20, Nc=70, D=1)
    ep = engine_of(zp)
    one = draws_of(zp)
    rep = {k: v.expand((5,) + tuple(v.shape[1:])).clone() for k, v in one.items()}
    r1, r5 = phase_marginal(ep, one, bins=20, return_per_draw=True), phase_marginal(ep, rep, bins=20, return_per_draw=True)
    assert r5.n_draws == 5 and torch.equal(r5.per_draw[0], r5.per_draw[4]) and torch.equal(r5.per_draw[0], r1.per_draw[0])
    # (five equal terms are not one term times five to the last bit: the sums over the draws round)
    assert torch.allclose(r1.posterior, r5.posterior, rtol=4 * EPS32, atol=1e-30) and torch.allclose(r1.log_evidence, r5.log_evidence, rtol=0, atol=1e-9)
    eng.close(), ep.close()


def test_priors():
    from velocycle_amd.predictive import phase_log_prior, phase_marginal
    z = cut(load("vel_mf_dnu2"), Ng=20, Nc=100, D=2)
    # priors of every strength: none, moderate, and strong enough that t = m . u reaches -20
    z["in_phixy_prior"] = (z["in_phixy_prior"] * np.linspace(0.0, 20.0, 100)[:, None] / np.maximum(1e-6, np.hypot(*z["in_phixy_prior"].T))[:, None]).astype(np.float32)
    eng = engine_of(z)
    dr = draws_of(z)
    B = 48
    flat = phase_marginal(eng, dr, bins=B, phase_prior="flat", return_per_draw=True)
    table = torch.full((100, B), -math.log(B), dtype=torch.float32)
    assert same_bits(flat, phase_marginal(eng, dr, bins=B, phase_prior=table, return_per_draw=True))
    model = phase_marginal(eng, dr, bins=B, phase_prior="model", return_per_draw=True)
    lw = phase_log_prior(torch.tensor(z["in_phixy_prior"]), B)
    assert bool(torch.isfinite(lw).all()) and float(lw.min()) < -150.0
    assert same_bits(model, phase_marginal(eng, dr, bins=B, phase_prior=lw, return_per_draw=True))
    assert same_bits(model, phase_marginal(eng, dr, bins=B, return_per_draw=True))                          # the default
    assert_within_bars("model prior", model, MC.evaluate(z, B, lw=lw.float().double().numpy()))            # the host's own lw, as the device reads it
    assert not torch.equal(model.posterior, flat.posterior)
    eng.close()


def test_extreme_counts_stay_finite_and_within_the_bars():
    from velocycle_amd.predictive import phase_marginal
    z = cut(load("phase_nb"), Ng=7, Nc=65, D=2)
    p = MC.PC.problem_of(z)
    mS, _ = MC.means(p, torch.zeros(65, dtype=torch.float64), 0)
    S = z["in_S"].copy()
    low = int(mS.mean(1).argmin())
    S[low, [0, 31, 64]] = 60000.0                                            # three cells of the lowest-expressed gene
    gi, ci = np.unravel_index(np.argsort(mS.numpy(), axis=None)[-5:], mS.shape)
    S[gi, ci] = 0.0                                                          # zeros where the mean is largest
    z["in_S"] = S
    eng = engine_of(z)
    rec = phase_marginal(eng, draws_of(z), bins=32, phase_prior="flat", return_per_draw=True)
    e64 = MC.evaluate(z, 32)
    assert float(e64["evidence"][0]) < -1e5                                  # every a of such a cell is below -1e5
    assert_within_bars("extremes", rec, e64)
    eng.close()


@pytest.mark.parametrize("case,noise", [("phase_poisson", "Poisson"), ("phase_nb", "NegativeBinomial")])
def test_against_the_independent_kernel_vc_phase_mle(case, noise):
    """The phase model under one draw and a flat prior is what vc_phase_mle scores (T = basis nu, m = exp(count_factor), one
    dispersion): log post_j - log post_best against its profile, within the sum of both kernels' bars -- on the bins whose posterior
    mass is a normal float32 (post >= 1e-30; a smaller mass has no logarithm to compare: float32 ends at 1e-38) -- and the same
    arg-max bin unless the float64 checker's top two lie within that sum."""
    from velocycle_amd.phase_mle import phase_mle
    from velocycle_amd.predictive import phase_marginal
    B, disp = 64, 0.3
    z = cut(load(case), D=1)
    if noise == "NegativeBinomial":
        z["draw_shape_inv"] = np.full_like(z["draw_shape_inv"], disp)
    eng = engine_of(z)
    rec = phase_marginal(eng, draws_of(z), bins=B, phase_prior="flat")
    e64 = MC.evaluate(z, B)
    nu = torch.tensor(z["draw_ν"][0]).double()                               # (Ng, 2 H + 1)
    T = MC.PC.basis(MC.grid(B), int(z["in_H"]), 0) @ nu.T                    # (B, Ng)
    m = np.exp(z["in_count_factor"].astype(np.float64)).reshape(-1)
    S = np.ascontiguousarray(z["in_S"].T)
    best, prof = phase_mle(S, T, m, noisemodel=noise, dispersion=disp, return_profile=True)
    best, prof = best.cpu(), prof.cpu().double().T                           # (Nc,), (Nc, B)
    logP, absP = LC.logp64(S, T, m, 1.0, noise, disp)
    A_mle = torch.as_tensor(LC.judge(logP, absP, best.numpy())["A"]).double()
    post = rec.posterior.double()
    mine = post.argmax(1)
    top = post.gather(1, mine[:, None])
    b = bars()["post"]
    bar = LF.profile_bar() * EPS32 * A_mle[:, None] + b * (EPS32 * e64["A"][:, None] * 2 + EPS32 / post.clamp(min=1e-30) + EPS32 / top)
    ok = post >= 1e-30
    diff = ((torch.log(post.clamp(min=1e-30)) - torch.log(top)) - prof).abs()
    worst = float((diff / bar)[ok].max())
    print(f"{case}: log-posterior profile against vc_phase_mle, worst |difference| / (sum of the bars) {worst:.4f} over {int(ok.sum())} of {ok.numel()} bins")
    assert worst <= 1.0
    lp = torch.log(e64["post"])
    top2 = lp.topk(2, dim=1).values
    close = (top2[:, 0] - top2[:, 1]) <= bar.gather(1, mine[:, None])[:, 0]
    print(f"{case}: {int(close.sum())} of {close.numel()} cells have their top two bins within the bar of each other; "
          f"{int((mine != best).sum())} arg-max bins differ")
    assert bool(((mine == best) | close).all())
    eng.close()


@pytest.mark.parametrize("case,seed", CALIBRATION)
def test_calibration_on_the_device(case, seed):
    from velocycle_amd.predictive import phase_marginal
    z, jstar, wrong = simulated(case, seed)
    eng = engine_of(z)
    rec = phase_marginal(eng, draws_of(z), bins=CAL_BINS, phase_prior="flat")
    zs, zc = MC.pit_z(rec.posterior, jstar, seed), MC.pit_z(MC.evaluate(z, CAL_BINS)["post"], jstar, seed)
    print(f"{case}: calibration z on the device {zs:.2f}, checker {zc:.2f}")
    assert abs(zs) < Z_BAR, zs
    for name, zw in wrong:
        zd = MC.pit_z(phase_marginal(eng, draws_of(zw), bins=CAL_BINS, phase_prior="flat").posterior, jstar, seed)
        print(f"{case}: control '{name}' z on the device {zd:.1f}")
        assert zd > Z_BAR, (name, zd)
    eng.close()


def test_held_out_cells_are_scored_by_another_engine_s_draws():
    """The cells of a fixture split into two engines: gene-level draws from the guide of the first problem score the second engine's
    cells, which no fit has seen and which bring no ϕxy."""
    from velocycle_amd.predictive import compare_evidence, phase_marginal
    z0 = load("vel_mf_joint_nb")
    Nc = z0["in_S"].shape[1]
    seen, held = cut(z0, Ng=40, cell_index=np.arange(0, Nc // 2)), cut(z0, Ng=40, cell_index=np.arange(Nc // 2, Nc))
    e_seen, e_held = engine_of(seen), engine_of(held)
    e_seen.init_params()
    dr = {k: v.cpu() for k, v in e_seen.sample_posterior(["ν", "shape_inv", "logγg", "logβg", "νω"], 4, seed=9).items()}
    assert "ϕxy" not in dr
    rec = phase_marginal(e_held, dr, bins=32, phase_prior="flat", return_per_draw=True)
    zc = dict(held)
    for k in list(zc):
        if k.startswith("draw_"):
            del zc[k]
    for k, v in dr.items():
        zc["draw_" + k] = v.numpy()
    zc["n_draws"] = np.int64(4)
    assert_within_bars("held-out cells", rec, MC.evaluate(zc, 32))
    assert compare_evidence(rec, rec) == (0.0, 0.0)
    other = phase_marginal(e_held, {**dr, "ν": dr["ν"] * 0.5}, bins=32, phase_prior="flat")
    d, se = compare_evidence(rec, other)
    assert np.isfinite(d) and se > 0
    e_seen.close(), e_held.close()


def _direct_call(eng):
    import ctypes as C
    one = C.c_void_p(64)                    # never dereferenced: the call is refused before anything is launched
    return eng.lib.vc_phase_marginal(eng._h, 4, one, 0, one, one, one, 0, one, 0, one, 0, 32, None, 0, 64, one, None, None, None)


def test_lognormal_and_run_time_sized_engines_are_refused_by_name():
    from velocycle_amd import _lib
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.predictive import phase_marginal
    from velocycle_amd.workloads import make_phase_spec
    for kw, word in ((dict(noisemodel="Lognormal"), "Lognormal"), (dict(H=4), "H = 4")):
        eng = HipEngine(make_phase_spec(Nc=200, Ng=20, **kw), device=torch.device("cuda:0"))
        eng.init_params()
        draws = eng.sample_posterior(["ν"], 3, seed=1)
        with pytest.raises(NotImplementedError, match=word):
            phase_marginal(eng, draws)
        assert _direct_call(eng) == _lib.VC_ERR_UNSUPPORTED and word.encode() in eng.lib.vc_last_error(eng._h)
        assert b"vc_phase_marginal" in eng.lib.vc_last_error(eng._h)
        eng.close()
