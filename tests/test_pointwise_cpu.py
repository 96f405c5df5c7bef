"""CPU: the float64 checker of the pointwise predictive density (tests/pointwise_checker.py) against the stored output of the
reference's own model functions (tests/golden/ref_pointwise_*.npz, written by tests/golden/make_golden_pointwise.py); the public
face (refusals before any device work, compare()); the C ABI declaration, its binding and its argument checks."""
import ctypes as C
import glob
import os
import re
import subprocess
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import pointwise_checker as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(os.path.basename(p)[len("ref_pointwise_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ref_pointwise_*.npz")))
WANTED = ["phase_h2_poisson", "phase_nb", "phase_poisson", "vel_lrmn_cond", "vel_mf_dnu2", "vel_mf_joint_nb"]


def load(case):
    z = np.load(os.path.join(GOLDEN, f"ref_pointwise_{case}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def bars():
    """Per quantity: 4 x the worst ratio the float32 reference itself shows over the fixtures."""
    return {q: PC.SAFETY * max(float(load(c)["ref_err_" + q]) for c in CASES) for q in PC.QUANT}


@lru_cache(maxsize=None)
def checked(case):
    z = load(case)
    return z, PC.evaluate(z)


def stored_reference(z, e64):
    return {m: {q: {"gene": z[f"ref_{m}_{q}_gene"], "cell": z[f"ref_{m}_{q}_cell"]} for q in PC.QUANT} for m in e64}


def test_fixtures_present():
    assert CASES == WANTED
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_pointwise_{c}.npz")) < (1 << 20)
        z = load(c)
        S = z["in_S"]
        assert S.max() > 255 and (S[0] == 0).all(), c                       # counts above 255 and a gene of zeros
        assert 8 <= int(z["n_draws"]) <= 16 and max(v.shape[0] for k, v in z.items() if k.startswith("draw_")) == int(z["n_draws"])
    z = load("vel_lrmn_cond")                                               # the tutorial conditioning: S is the same in every draw
    assert z["draw_ϕxy"].shape[0] == 1 and z["draw_ν"].shape[0] == 1 and z["draw_logγg"].shape[0] == 16 and int(z["in_Hw"]) == 1
    assert load("vel_mf_dnu2")["in_Db"].shape[0] == 2 and int(load("phase_h2_poisson")["in_H"]) == 2


@pytest.mark.parametrize("case", WANTED)
def test_checker_against_stored_reference(case):
    z, e64 = checked(case)
    for m in e64:
        for q in PC.QUANT:
            assert bool(torch.isfinite(e64[m][q]).all()) and bool((e64[m]["A"] > 0).all()), (case, m, q)
    r = PC.ratios(stored_reference(z, e64), e64)
    worst = max(r.values()) * PC.EPS32
    print(f"{case}: checker vs the stored float64 reference {worst:.2e} A; stored float32 reference ratios",
          {q: round(float(z['ref_err_' + q]), 3) for q in PC.QUANT})
    assert worst <= 1e-10, (case, r)
    # the checker's own float32 evaluation lands in the same band as the reference's
    r32 = PC.ratios(PC.as_got({m: {q: v[q].double() for q in PC.QUANT} for m, v in PC.evaluate(z, torch.float32).items()}), e64)
    assert all(np.isfinite(v) and v < PC.SANITY for v in r32.values()), (case, r32)


def test_bars_come_from_the_reference():
    b = bars()
    print("bars (eps32 A):", b)
    assert all(np.isfinite(v) and 0 < v < PC.SANITY for v in b.values()), b
    for c in CASES:
        for q in PC.QUANT:
            assert 0 < float(load(c)["ref_err_" + q]) < PC.SANITY, (c, q)


def test_checker_identities_on_a_planted_case():
    g = torch.Generator().manual_seed(5)
    l1 = 40.0 * torch.randn((1, 7, 9), generator=g, dtype=torch.float64) - 100.0
    lppd, mean, pw = PC.reduce_draws(l1.expand(6, 7, 9).clone())                 # all draws equal
    assert torch.equal(lppd, mean) and torch.equal(mean, l1[0]) and bool((pw == 0).all())
    # two draws a and b: log((e^a + e^b) / 2), (a + b) / 2, (a - b)^2 / 2 -- also 700 apart, where exp underflows without the shift
    a = torch.tensor([[[-3.0, -800.0, 2.5]]], dtype=torch.float64)
    b = torch.tensor([[[-1.0, -100.0, 2.5]]], dtype=torch.float64)
    lppd, mean, pw = PC.reduce_draws(torch.cat([a, b]))
    want = torch.maximum(a, b)[0] + torch.log1p(torch.exp(-(a - b).abs()[0])) - np.log(2.0)
    assert torch.allclose(lppd, want, rtol=0, atol=1e-12) and bool(torch.isfinite(lppd).all())
    assert torch.allclose(mean, (a + b)[0] / 2) and torch.allclose(pw, ((a - b)[0] ** 2) / 2)
    # the whole evaluation with every draw equal: pwaic 0, lppd == mean
    z = load("phase_poisson")
    for k in list(z):
        if k.startswith("draw_"):
            z[k] = np.repeat(z[k][:1], 4, axis=0)
    e = PC.evaluate(z)["S"]
    assert torch.equal(e["lppd"], e["mean"]) and bool((e["pwaic"] == 0).all())


def test_header_declares_and_lib_binds_vc_pointwise_density():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    m = re.search(r"\bint vc_pointwise_density\(vc_engine\* e, int64_t n_draws,([^;]*)\);", hdr)
    assert m, "vc_pointwise_density is not declared"
    arity = 2 + m.group(1).count(",") + 1
    assert "vc_pointwise_density" in _lib.EXPORTS and len(_lib.EXPORTS["vc_pointwise_density"][1]) == arity == 20
    assert "#define VC_ABI_VERSION 2" in hdr and _lib.VC_ABI_VERSION == 2
    assert "velocity_inference_model.py:338-386" in hdr and "lgamma(r+k) - lgamma(r) - lgamma(k+1)" in hdr


def _fake_engine(noise="NegativeBinomial", kind="velocity"):
    spec = types.SimpleNamespace(kind=kind, noisemodel=noise, Ng=5, Nc=8, H=1, Hw=1, Nh=3, Nhw=3, Nb=1, Nx=1, with_delta_nu=False,
                                 condition_on={})
    return types.SimpleNamespace(spec=spec, Nc_local=8)


def test_refusals_fire_before_the_device(monkeypatch):
    from velocycle_amd import _lib, predictive
    from velocycle_amd.fit_models import PhaseFitModel, VelocityFitModel

    def no_device(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "synchronize", no_device)
    draws = {"ν": torch.zeros(4, 5, 3), "ϕxy": torch.ones(4, 8, 2)}
    with pytest.raises(NotImplementedError, match="Lognormal"):
        predictive.pointwise_density(_fake_engine("Lognormal"), draws)
    with pytest.raises(ValueError, match="at least 2 draws"):
        predictive.pointwise_density(_fake_engine(), {k: v[:1] for k, v in draws.items()})
    with pytest.raises(ValueError, match="'ν' and 'ϕxy'"):
        predictive.pointwise_density(_fake_engine(), {"ν": draws["ν"]})
    big = _fake_engine()
    big.spec.Ng, big.Nc_local = 40000, 40000
    with pytest.raises(ValueError, match="return_pointwise"):
        predictive.pointwise_density(big, {"ν": torch.zeros(2, 1, 1), "ϕxy": torch.zeros(2, 1, 2)}, return_pointwise=True)
    # the fit drivers: not fitted; Lognormal / too few draws on a fitted-looking model
    mp = types.SimpleNamespace(model_fn=None, guide_fn=None)
    for cls in (PhaseFitModel, VelocityFitModel):
        with pytest.raises(ValueError, match="not been fitted"):
            cls(mp).predictive_density()
        f = cls(mp)
        f.engine, f.losses, f.spec = _fake_engine("Lognormal"), [1.0], _fake_engine("Lognormal").spec
        with pytest.raises(NotImplementedError, match="Lognormal"):
            f.predictive_density()
        f.engine, f.spec = _fake_engine(), _fake_engine().spec
        with pytest.raises(ValueError, match="at least 2 draws"):
            f.predictive_density(num_samples=1)


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)                    # never dereferenced: every call below is refused before anything is launched

    def call(e, n_draws=4, gene=one, cell=one, phixy=one):
        return lib.vc_pointwise_density(e, n_draws, phixy, 0, one, 0, None, one, None, 0, None, 0, None, 0, 0, 8, gene, cell, None, None)
    assert call(None) == _lib.VC_ERR_ARG and b"null engine" in lib.vc_last_error(None)
    cfg = _lib.vc_config(abi_version=_lib.VC_ABI_VERSION, model=0, guide=0, noise=0, with_delta_nu=0, n_harmonics=1, n_harmonics_w=0,
                         Nb=1, Nx=0, lrmn_rank=5, rank=0, world_size=1, Ng=5, Nc_local=8, Nc_global=8, cell_offset=0, gamma_alpha=1.0,
                         gamma_beta=2.0, sigma_ln_s=0.5, sigma_ln_u=0.1, rho_mean=4.0, rho_std=1.0, rho_scale=1.0)
    h = C.c_void_p()
    assert lib.vc_create(C.byref(cfg), C.byref(h)) == _lib.VC_OK
    try:
        assert call(h, n_draws=1) == _lib.VC_ERR_ARG and b"n_draws" in lib.vc_last_error(h)
        assert call(h, n_draws=0) == _lib.VC_ERR_ARG
        assert call(h, gene=None) == _lib.VC_ERR_ARG and b"null gene_out_dev" in lib.vc_last_error(h)
        assert call(h, cell=None) == _lib.VC_ERR_ARG
        assert call(h) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
        # a call that one of the refusals shared with vc_predictive_check would stop too (null phixy) still meets the entry point's
        # own refusals first, in their order
        assert call(h, n_draws=1, phixy=None) == _lib.VC_ERR_ARG and b"n_draws must be >= 2" in lib.vc_last_error(h)
        assert call(h, gene=None, phixy=None) == _lib.VC_ERR_ARG and b"null gene_out_dev" in lib.vc_last_error(h)
        assert call(h, phixy=None) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
    finally:
        lib.vc_destroy(h)


def _record(cell_s, cell_u=None, pw=0.0):
    from velocycle_amd.predictive import PredictiveDensity
    mk = lambda v: {"S": torch.tensor(v, dtype=torch.float64), **({"U": torch.tensor(cell_u, dtype=torch.float64)} if cell_u is not None else {})}
    zeros = lambda v: {k: torch.full_like(t, pw) for k, t in mk(v).items()}
    g = {k: torch.zeros(3, dtype=torch.float64) for k in mk(cell_s)}
    return PredictiveDensity(lppd_gene=g, lppd_cell=mk(cell_s), mean_gene=g, mean_cell=mk(cell_s), p_waic_gene=g, p_waic_cell=zeros(cell_s),
                             n_draws=4)


def test_compare_on_hand_made_records():
    from velocycle_amd.predictive import compare
    a = _record([-1.0, -2.0, -3.0, -4.0], [-1.0, -1.0, -1.0, -1.0], pw=0.5)
    b = _record([-2.0, -2.0, -5.0, -4.5], [-1.0, -2.0, -1.0, -1.5], pw=0.25)
    # per cell: (lppd - p_waic) added over the matrices
    diff = np.array([1.0, 1.0, 2.0, 1.0]) - 2 * 0.25
    d, se = compare(a, b)
    assert d == pytest.approx(diff.sum()) and se == pytest.approx(np.sqrt(4 * diff.var(ddof=1)))
    d2, se2 = compare(b, a)
    assert d2 == pytest.approx(-d) and se2 == pytest.approx(se)
    assert a.elpd_waic == pytest.approx(-14.0 - 8 * 0.5) and a.waic == pytest.approx(-2 * a.elpd_waic)
    assert a.lppd == pytest.approx(-14.0) and a.p_waic == pytest.approx(4.0)
    with pytest.raises(ValueError, match="same cells"):
        compare(a, _record([-1.0, -2.0, -3.0], [-1.0, -1.0, -1.0]))


def test_library_builds_and_the_kernel_has_no_scratch(tmp_path):
    """The new translation unit compiles for gfx950 and every instantiation of the element kernel reports
    .private_segment_fixed_size 0 in the metadata of the emitted assembly (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_pointwise.hip")
    out = str(tmp_path / "pw.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.name:\s+(\S*vc_pointwise_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", txt)
    assert len(found) == 36, len(found)                    # H 1..3 x {phase, velocity, velocity with S hoisted} x {NB, Poisson} x {u16, f32}
    assert all(int(n) == 0 for _, n in found), [f for f in found if int(f[1])]
