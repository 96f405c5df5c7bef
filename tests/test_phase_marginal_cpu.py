"""CPU: the float64 checker of phase-marginal scoring (tests/phase_marginal_checker.py) -- its float32 restatement on the fixtures of the
reference's own model (tests/golden/ref_pointwise_*.npz), which defines the bars of the GPU tests, and its calibration on counts
simulated from the model; the projected-normal phase prior; the public face (refusals before any device work, the record's
arithmetic, merge, compare_evidence, Phases.from_phase_marginal); the C ABI declaration and its argument checks; no scratch."""
import ctypes as C
import math
import os
import re
import subprocess
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import phase_marginal_checker as MC
from tests import pointwise_checker as PC
from tests.test_pointwise_cpu import CASES, WANTED, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_FIXTURES = 32
Z_BAR = 6.0                      # the project's bar of a chi-square z-score (tests/test_hip_pit.py, tests/test_hip_ppc.py)
CALIBRATION = (("phase_h2_poisson", 11), ("vel_lrmn_cond", 12))       # (fixture, seed of the simulation)
CAL_BINS = 64


@lru_cache(maxsize=None)
def checked(case, B=B_FIXTURES):
    z = load(case)
    return z, MC.evaluate(z, B)


@lru_cache(maxsize=None)
def float32_ratios():
    """{case: {quantity: worst ratio}} of the checker's own float32 evaluation against its float64 one, B = 32, flat prior."""
    out = {}
    for c in CASES:
        z, e64 = checked(c)
        e32 = MC.evaluate(z, B_FIXTURES, dtype=torch.float32)
        out[c] = MC.ratios({q: e32[q].double() for q in MC.QUANT}, e64)
    return out


def bars():
    """Per quantity: 4 x the worst ratio the float32 restatement shows over the fixtures (computed, not stored)."""
    r = float32_ratios()
    return {q: PC.SAFETY * max(r[c][q] for c in CASES) for q in MC.QUANT}


@lru_cache(maxsize=None)
def simulated(case, seed):
    """(simulated fixture, true bins, [(control name, fixture)]) of a calibration case."""
    z, jstar = MC.simulate(load(case), CAL_BINS, seed)
    return z, jstar, MC.wrong_models(z)


def test_float32_restatement_defines_the_bars():
    assert CASES == WANTED
    r = float32_ratios()
    for c in CASES:
        z, e64 = checked(c)
        assert all(bool(torch.isfinite(e64[q]).all()) for q in MC.QUANT) and bool((e64["A"] > 0).all()), c
        assert torch.allclose(e64["post"].sum(1), torch.ones(e64["post"].shape[0], dtype=torch.float64), rtol=0, atol=1e-12)
        print(f"{c}: float32 restatement ratios " + ", ".join(f"{q} {r[c][q]:.4f}" for q in MC.QUANT) +
              f"; evidence abs err <= {r[c]['evidence'] * MC.EPS32 * float(e64['A'].max()):.1e}; A in [{float(e64['A'].min()):.0f}, {float(e64['A'].max()):.0f}]")
        assert all(np.isfinite(v) and 0 < v < PC.SANITY for v in r[c].values()), (c, r[c])
    b = bars()
    print("bars (units of the checker):", b)
    assert all(np.isfinite(v) and 0 < v < PC.SAFETY * PC.SANITY for v in b.values())


def test_checker_identities():
    z = load("phase_poisson")
    e = MC.evaluate(z, 8)
    D = int(z["n_draws"])
    # evidence = log mean_d exp per_draw;  post = the draws' posteriors weighted by their evidences
    assert torch.allclose(e["evidence"], torch.logsumexp(e["per_draw"], 0) - math.log(D), rtol=0, atol=1e-9)
    # equal draws: evidence == per_draw of any draw; a prior that is -inf outside one bin puts the whole posterior there
    for k in list(z):
        if k.startswith("draw_"):
            z[k] = np.repeat(z[k][:1], 3, axis=0)
    z["n_draws"] = np.int64(3)
    e1 = MC.evaluate(z, 8)
    assert torch.allclose(e1["evidence"], e1["per_draw"][0], rtol=0, atol=1e-9) and torch.equal(e1["per_draw"][0], e1["per_draw"][2])
    Nc = z["in_S"].shape[1]
    lw = np.full((Nc, 8), -1e6)
    lw[:, 3] = 0.0
    e2 = MC.evaluate(z, 8, lw=lw)
    assert bool((e2["post"][:, 3] == 1.0).all()) and bool(torch.isfinite(e2["evidence"]).all())
    # with the cells' directions on the grid, the pointwise checker's own sum over genes is the a of that bin
    p = PC.problem_of(z)
    j = np.arange(Nc) % 8
    ph = MC.grid(8)[j]
    p["draws"]["ϕxy"] = torch.stack([torch.cos(ph), torch.sin(ph)], -1).expand(3, Nc, 2)
    want = PC.log_probs(p)["S"][0].sum(1)
    tot, _ = MC.gene_sums(PC.problem_of(z), 8)
    assert torch.allclose(tot[:, torch.arange(Nc), torch.as_tensor(j)], want, rtol=1e-13, atol=1e-9)


@pytest.mark.parametrize("case,seed", CALIBRATION)
def test_checker_is_calibrated_on_simulated_counts(case, seed):
    """Counts simulated from the model with every cell's true phase on the grid (one draw, B = 64, flat prior): the randomized PIT of
    the true bin under the checker's posterior is uniform (|z| < 6 of its 10-bin chi-square); under the two wrong models it is not."""
    z, jstar, wrong = simulated(case, seed)
    e = MC.evaluate(z, CAL_BINS)
    zs = MC.pit_z(e["post"], jstar, seed)
    hit = float((e["post"].argmax(1) == jstar).double().mean())
    print(f"{case}: calibration z {zs:.2f} ({z['in_S'].shape[1]} cells; the MAP bin is the true one in {100 * hit:.0f} %)")
    assert abs(zs) < Z_BAR, zs
    for name, zw in wrong:
        zc = MC.pit_z(MC.evaluate(zw, CAL_BINS)["post"], jstar, seed)
        print(f"{case}: control '{name}' z {zc:.1f}")
        assert zc > Z_BAR, (name, zc)


# ----------------------------------------------------------------------------------------------------------------------------------
# the projected-normal prior
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [0.0, 0.5, 5.0, 10.0, 30.0])
def test_projected_normal_integrates_to_one(norm):
    from velocycle_amd.predictive import phase_grid, projected_normal_logpdf
    B = 4096
    for ang in (0.0, 0.7, 4.0):
        m = torch.tensor([norm * math.cos(ang), norm * math.sin(ang)], dtype=torch.float64)
        lp = projected_normal_logpdf(m[None, :], phase_grid(B))
        assert bool(torch.isfinite(lp).all())
        mass = float(torch.exp(lp).sum() * (2 * math.pi / B))
        assert abs(mass - 1.0) < 1e-9, (norm, ang, mass)


def test_projected_normal_against_radial_quadrature():
    """p(phi) = int_0^inf r N((r cos phi, r sin phi); m, I) dr, by a fine trapezoid rule, at a handful of angles -- among them ones where
    t = m . u is very negative (the cancelling branch and its asymptotic series)."""
    from velocycle_amd.predictive import projected_normal_logpdf
    r = torch.linspace(0.0, 60.0, 600001, dtype=torch.float64)
    for m in ([0.0, 0.0], [0.3, -0.4], [3.0, 4.0], [-6.0, 8.0], [0.0, 13.0], [20.0, -22.0]):
        mt = torch.tensor(m, dtype=torch.float64)
        for phi in (0.0, 1.0, 2.5, 4.0, 5.5):
            u = torch.tensor([math.cos(phi), math.sin(phi)], dtype=torch.float64)
            t = float(mt @ u)
            # log integrand, shifted by its maximum: -|r u - m|^2 / 2 = -(r - t)^2 / 2 - (|m|^2 - t^2) / 2
            logf = torch.log(r.clamp(min=1e-300)) - 0.5 * (r - t) ** 2
            shift = float(logf.max())
            quad = math.log(float(torch.trapezoid(torch.exp(logf - shift), r))) + shift - 0.5 * (float(mt @ mt) - t * t) - math.log(2 * math.pi)
            got = float(projected_normal_logpdf(mt, torch.tensor(phi, dtype=torch.float64)))
            assert abs(got - quad) < 1e-7 * max(1.0, abs(quad)), (m, phi, t, got, quad)          # (the quadrature's own error: h^2 f'' / 12)


def test_phase_log_prior_and_concentration_inversion():
    from velocycle_amd.predictive import concentration_of_resultant, phase_grid, phase_log_prior, projected_normal_resultant
    m = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, -3.0], [-20.0, 20.0]])
    lw = phase_log_prior(m, 128)
    assert lw.dtype == torch.float64 and lw.shape == (4, 128) and bool(torch.isfinite(lw).all())
    assert torch.allclose(torch.exp(lw).sum(1), torch.ones(4, dtype=torch.float64), rtol=0, atol=1e-12)
    assert torch.allclose(lw[0], torch.full((128,), -math.log(128.0), dtype=torch.float64), rtol=0, atol=1e-12)
    assert int(lw[1].argmax()) == 0 and int(lw[2].argmax()) == 96 and int(lw[3].argmax()) == 48
    # the closed form of the resultant length against the grid's own, and its inversion
    ph = phase_grid(4096)
    for k in (0.1, 1.0, 3.0, 10.0):
        p = torch.exp(phase_log_prior(torch.tensor([[k, 0.0]]), 4096))[0]
        R = float(torch.sqrt((p @ torch.cos(ph)) ** 2 + (p @ torch.sin(ph)) ** 2))
        assert abs(float(projected_normal_resultant(k)) - R) < 1e-9, (k, R)
        assert abs(float(concentration_of_resultant(R)) - k) < 1e-6 * max(1.0, k)
    assert float(concentration_of_resultant(0.0)) < 1e-9


# ----------------------------------------------------------------------------------------------------------------------------------
# the public face
# ----------------------------------------------------------------------------------------------------------------------------------
def _record(ev, post, per_draw=None, n_draws=3):
    from velocycle_amd.predictive import PhaseMarginal, phase_grid
    post = torch.tensor(post, dtype=torch.float32)
    return PhaseMarginal(log_evidence=torch.tensor(ev, dtype=torch.float64), posterior=post, phis=phase_grid(post.shape[1]), n_draws=n_draws,
                         per_draw=None if per_draw is None else torch.tensor(per_draw, dtype=torch.float64))


def test_record_arithmetic_merge_and_compare():
    from velocycle_amd.predictive import compare_evidence, merge_marginal_shards
    a = _record([-10.0, -20.0, -30.0], [[1, 0, 0, 0], [0.5, 0, 0.5, 0], [0.25, 0.25, 0.25, 0.25]], per_draw=[[-9.0, -19.0, -29.0]] * 3)
    assert a.elpd == pytest.approx(-60.0)
    assert a.mean_phase[0].item() == pytest.approx(0.0) and a.resultant_length.tolist() == pytest.approx([1.0, 0.0, 0.0], abs=1e-12)
    assert a.entropy.tolist() == pytest.approx([0.0, math.log(2.0), math.log(4.0)]) and a.map_phase[0].item() == 0.0
    q = _record([-1.0], [[0, 0.5, 0.5, 0]])
    assert q.mean_phase[0].item() == pytest.approx(0.75 * math.pi) and q.resultant_length[0].item() == pytest.approx(math.sqrt(0.5))
    assert _record([-1.0], [[0, 0, 0, 1.0]]).mean_phase[0].item() == pytest.approx(1.5 * math.pi)          # in [0, 2 pi)
    b = _record([-11.0], [[0, 1, 0, 0]], per_draw=[[-1.0]] * 3)
    got = merge_marginal_shards([a, b])
    assert got.log_evidence.tolist() == [-10.0, -20.0, -30.0, -11.0] and got.posterior.shape == (4, 4) and got.per_draw.shape == (3, 4)
    assert got.posterior[3].tolist() == [0, 1, 0, 0] and got.n_draws == 3 and torch.equal(got.phis, a.phis)
    with pytest.raises(ValueError, match="different draws or grids"):
        merge_marginal_shards([a, _record([-1.0], [[1, 0, 0, 0]], per_draw=[[-1.0]] * 3, n_draws=2)])
    with pytest.raises(ValueError, match="different draws or grids"):
        merge_marginal_shards([a, _record([-1.0], [[1, 0]], per_draw=[[-1.0]] * 3)])
    with pytest.raises(ValueError, match="only some"):
        merge_marginal_shards([a, _record([-1.0], [[1, 0, 0, 0]])])
    # compare_evidence: the paired difference over cells and sqrt(n var) of it
    c = _record([-11.0, -20.5, -28.0], [[1, 0, 0, 0]] * 3)
    diff = np.array([1.0, 0.5, -2.0])
    d, se = compare_evidence(a, c)
    assert d == pytest.approx(diff.sum()) and se == pytest.approx(math.sqrt(3 * diff.var(ddof=1)))
    d2, se2 = compare_evidence(c, a)
    assert d2 == pytest.approx(-d) and se2 == pytest.approx(se)
    assert compare_evidence(a, a) == (0.0, 0.0)
    with pytest.raises(ValueError, match="same cells"):
        compare_evidence(a, b)


def test_phases_from_phase_marginal():
    from velocycle_amd.containers import Phases
    from velocycle_amd.predictive import phase_log_prior, projected_normal_resultant
    rec = _record([-1.0, -2.0], [[0, 1, 0, 0], [0.5, 0, 0, 0.5]])
    ph = Phases.from_phase_marginal(rec, cell_names=["a", "b"], concentration=4.0)
    assert list(ph.phi_xy.columns) == ["a", "b"] and ph.phi_xy.shape == (2, 2)
    assert ph.phi_xy.values[:, 0] == pytest.approx([0.0, 4.0], abs=1e-12)
    assert ph.phi_xy.values[:, 1] == pytest.approx([4.0 * math.cos(-math.pi / 4), 4.0 * math.sin(-math.pi / 4)], abs=1e-12)
    # without a concentration: the kappa whose projected normal has the posterior's resultant length -- a posterior that IS a projected
    # normal on a fine grid gives its own mean vector back
    m = torch.tensor([[2.0, -1.0], [-0.3, 0.4]], dtype=torch.float64)
    post = torch.exp(phase_log_prior(m, 2048))
    rec = _record([-1.0, -2.0], post.tolist())
    got = Phases.from_phase_marginal(rec).phi_xy.values.T
    assert np.abs(got - m.numpy()).max() < 1e-4, got
    assert np.allclose(np.hypot(got[:, 0], got[:, 1]), [math.sqrt(5.0), 0.5], atol=1e-4)
    assert float(projected_normal_resultant(math.sqrt(5.0))) == pytest.approx(float(rec.resultant_length[0]), abs=1e-6)


def _fake_engine(noise="NegativeBinomial", kind="velocity", generic=False):
    spec = types.SimpleNamespace(kind=kind, noisemodel=noise, Ng=5, Nc=8, H=1, Hw=1, Nh=3, Nhw=3, Nb=1, Nx=1, with_delta_nu=False,
                                 condition_on={}, phixy_prior=torch.zeros(8, 2))
    return types.SimpleNamespace(spec=spec, Nc_local=8, c0=0, c1=8, stats={"generic": generic})


def test_refusals_fire_before_the_device(monkeypatch):
    from velocycle_amd import _lib, predictive
    from velocycle_amd.fit_models import PhaseFitModel, VelocityFitModel

    def no_device(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    draws = {"ν": torch.zeros(4, 5, 3)}                                      # no ϕxy: not required here
    with pytest.raises(NotImplementedError, match="Lognormal"):
        predictive.phase_marginal(_fake_engine("Lognormal"), draws)
    for bad in (1, 4097, 0, 12.5):
        with pytest.raises(ValueError, match="bins must be an integer in"):
            predictive.phase_marginal(_fake_engine(), draws, bins=bad)
    with pytest.raises(ValueError, match=r"prior tensor has shape \(8, 15\), expected \(8, 16\)"):
        predictive.phase_marginal(_fake_engine(), draws, bins=16, phase_prior=torch.zeros(8, 15))
    with pytest.raises(ValueError, match=r"expected \(8, 16\)"):
        predictive.phase_marginal(_fake_engine(), draws, bins=16, phase_prior=torch.zeros(7, 16))
    with pytest.raises(ValueError, match="phase_prior must be one of"):
        predictive.phase_marginal(_fake_engine(), draws, phase_prior="uniform")
    with pytest.raises(NotImplementedError, match="run-time-sized kernel set"):
        predictive.phase_marginal(_fake_engine(generic=True), draws)
    with pytest.raises(ValueError, match="at least the site 'ν'"):
        predictive.phase_marginal(_fake_engine(), {"ϕxy": torch.zeros(4, 8, 2)})
    # the number of draws does not come from ϕxy; the other entry points still ask for it
    assert predictive._draw_count({"ν": torch.zeros(1, 5, 3), "ϕxy": torch.zeros(9, 8, 2)}, phixy=False) == 1
    assert predictive._draw_count({"ν": torch.zeros(1, 5, 3), "ϕxy": torch.zeros(9, 8, 2)}) == 9
    with pytest.raises(ValueError, match="'ν' and 'ϕxy'"):
        predictive._draw_count(draws)
    mp = types.SimpleNamespace(model_fn=None, guide_fn=None)
    for cls in (PhaseFitModel, VelocityFitModel):
        with pytest.raises(ValueError, match="not been fitted"):
            cls(mp).phase_marginal()
        f = cls(mp)
        f.engine, f.losses, f.spec = _fake_engine("Lognormal"), [1.0], _fake_engine("Lognormal").spec
        with pytest.raises(NotImplementedError, match="Lognormal"):
            f.phase_marginal()
        f.engine, f.spec = _fake_engine(), _fake_engine().spec
        with pytest.raises(ValueError, match="bins must be an integer in"):
            f.phase_marginal(bins=5000)
        with pytest.raises(ValueError, match="at least 1 draw"):
            f.phase_marginal(num_samples=0)


def test_header_declares_and_lib_binds_vc_phase_marginal():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    m = re.search(r"\bint vc_phase_marginal\(vc_engine\* e, int64_t n_draws,([^;]*)\);", hdr)
    assert m, "vc_phase_marginal is not declared"
    arity = 2 + m.group(1).count(",") + 1
    assert "vc_phase_marginal" in _lib.EXPORTS and len(_lib.EXPORTS["vc_phase_marginal"][1]) == arity == 20
    assert "#define VC_ABI_VERSION 2" in hdr and _lib.VC_ABI_VERSION == 2
    assert "phixy" not in m.group(1) and "int32_t n_bins, const float* log_prior_dev" in m.group(1)
    # the draw arguments are those of vc_pointwise_density without phixy and its stride, in their order
    pw, pm = _lib.EXPORTS["vc_pointwise_density"][1], _lib.EXPORTS["vc_phase_marginal"][1]
    assert pm[:2] == pw[:2] and pm[2:12] == pw[4:14] and pm[12] == C.c_int32
    doc = hdr.split("int vc_phase_marginal(")[0].split("phase-marginal scoring")[-1]
    assert "phases.py:471-509" in doc and "phases.py:495" in doc and "velocity_inference_model.py:338-386" in doc and "discrete grid" in doc


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)                    # never dereferenced: every call below is refused before anything is launched

    def call(e, n_draws=4, bins=32, evidence=one, nu=one):
        return lib.vc_phase_marginal(e, n_draws, nu, 0, None, one, None, 0, None, 0, None, 0, bins, None, 0, 8, evidence, None, None, None)
    assert call(None) == _lib.VC_ERR_ARG and b"null engine" in lib.vc_last_error(None)
    cfg = _lib.vc_config(abi_version=_lib.VC_ABI_VERSION, model=0, guide=0, noise=0, with_delta_nu=0, n_harmonics=1, n_harmonics_w=0,
                         Nb=1, Nx=0, lrmn_rank=5, rank=0, world_size=1, Ng=5, Nc_local=8, Nc_global=8, cell_offset=0, gamma_alpha=1.0,
                         gamma_beta=2.0, sigma_ln_s=0.5, sigma_ln_u=0.1, rho_mean=4.0, rho_std=1.0, rho_scale=1.0)
    h = C.c_void_p()
    assert lib.vc_create(C.byref(cfg), C.byref(h)) == _lib.VC_OK
    try:
        assert call(h, n_draws=0) == _lib.VC_ERR_ARG and b"n_draws must be >= 1" in lib.vc_last_error(h)
        assert call(h, n_draws=(1 << 20) + 1) == _lib.VC_ERR_ARG and b"2^20" in lib.vc_last_error(h)
        for bad in (1, 4097, 0, -1):
            assert call(h, bins=bad) == _lib.VC_ERR_ARG and b"n_bins must lie in [2, 4096]" in lib.vc_last_error(h)
        assert call(h, evidence=None) == _lib.VC_ERR_ARG and b"null evidence_dev" in lib.vc_last_error(h)
        assert call(h) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
        # the entry point's own refusals come before the ones it shares with its neighbours (null nu), in their order
        assert call(h, n_draws=0, nu=None) == _lib.VC_ERR_ARG and b"n_draws must be >= 1" in lib.vc_last_error(h)
        assert call(h, nu=None) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
    finally:
        lib.vc_destroy(h)
    eng = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_engine.hip")).read()
    body = eng[eng.index('extern "C" int vc_phase_marginal'):]
    assert body.index("draw_args(e,") < body.index("hipMemcpy") < body.index("vc_launch_phase_marginal")       # refused before any device work


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_phase_marginal_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly emitted for
    gfx950 (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_phase_marginal.hip")
    out = str(tmp_path / "pm.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.name:\s+(\S*vc_phase_marginal_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", txt)
    assert len(found) == 24, len(found)                    # H 1..3 x {phase, velocity} x {NB, Poisson} x {u16, f32}
    assert all(int(n) == 0 for _, n in found), [f for f in found if int(f[1])]
