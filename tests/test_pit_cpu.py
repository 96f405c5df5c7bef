"""CPU: the float64 checker of the predictive PIT (tests/pit_checker.py) against scipy's CDFs on the pointwise fixtures
(tests/golden/ref_pointwise_*.npz); the measured bar of the GPU tests; calibration of the checker on scipy-sampled counts; the public
face (refusals before any device work, merge_pit_shards, the summaries); the C ABI declaration, its binding and its argument checks;
the code object (no scratch)."""
import ctypes as C
import os
import re
import subprocess
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import pit_checker as Q
from tests.test_pointwise_cpu import CASES, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11


@lru_cache(maxsize=None)
def checked(case):
    """The fixture and its float64 evaluation under SEED, computed once and shared (do not modify)."""
    z = load(case)
    return z, Q.evaluate(z, SEED)


@lru_cache(maxsize=None)
def float32_ratios():
    """Per fixture the worst error ratio per quantity of the checker's own float32 evaluation."""
    out = {}
    for c in CASES:
        z, e64 = checked(c)
        out[c] = Q.ratios(Q.evaluate(z, SEED, torch.float32), e64)
    return out


def bars():
    """The bar of the GPU tests, in accuracy units: 4 x the worst ratio the float32 restatement itself shows over the fixtures (one
    number: F_lo, F_hi and u share the unit)."""
    return Q.SAFETY * max(max(r.values()) for r in float32_ratios().values())


@pytest.mark.parametrize("case", CASES)
def test_checker_against_scipy(case):
    st = pytest.importorskip("scipy.stats")
    z, e64 = checked(case)
    p = Q.PC.problem_of(z)
    nb = p["noise"] == "NegativeBinomial"
    for m, eta in Q.etas(p).items():
        mu = np.exp(eta.numpy())
        k = p[m].numpy()[None]
        if nb:
            r = (1.0 / p["draws"]["shape_inv"].numpy())[:, :, None]
            cdf = lambda q: st.nbinom.cdf(q, r, r / (r + mu))
        else:
            cdf = lambda q: st.poisson.cdf(q, mu)
        hi, lo = cdf(k).mean(0), cdf(k - 1).mean(0)
        got = e64[m]
        assert bool(torch.isfinite(got["F_lo"]).all()) and bool(torch.isfinite(got["F_hi"]).all())
        assert bool(((got["F_lo"] >= 0) & (got["F_lo"] <= got["F_hi"]) & (got["F_hi"] <= 1 + 1e-12)).all()), (case, m)
        tol = 1e-10 * (hi + 1e-300)
        for name, want in (("F_lo", lo), ("F_hi", hi)):
            err = np.abs(got[name].numpy() - want)
            print(f"{case} {m} {name}: worst |checker - scipy| / F_hi = {float((err / (hi + 1e-300)).max()):.2e}")
            assert bool((err <= tol).all()), (case, m, name, float((err / (hi + 1e-300)).max()))
        assert bool(((got["u"] >= got["F_lo"]) & (got["u"] <= got["F_hi"])).all()) and bool((got["s"] > 0).all())


def test_the_bar_is_measured_and_lies_in_the_sanity_band():
    r = float32_ratios()
    for c in CASES:
        print(f"{c}: float32 restatement, error ratios " + ", ".join(f"{q} {r[c][q]:.3f}" for q in Q.QUANT))
    b = bars()
    print(f"bar of the GPU tests: {b:.3f} accuracy units")
    assert np.isfinite(b) and 0 < b < Q.SANITY, b


def _resampled(case, rng_seed):
    """Draw 0 of the fixture with its counts replaced by scipy samples from that draw's own likelihood."""
    st = pytest.importorskip("scipy.stats")
    from tests.test_hip_pointwise import cut
    z = cut(load(case), D=1)
    p = Q.PC.problem_of(z)
    rng = np.random.default_rng(rng_seed)
    for m, eta in Q.etas(p).items():
        mu = np.exp(eta.numpy()[0])
        if p["noise"] == "NegativeBinomial":
            r = (1.0 / p["draws"]["shape_inv"].numpy()[0])[:, None]
            k = st.nbinom.rvs(r, r / (r + mu), size=mu.shape, random_state=rng)
        else:
            k = st.poisson.rvs(mu, size=mu.shape, random_state=rng)
        z["in_" + m] = k.astype(np.float32)
    return z


@pytest.mark.parametrize("case", ["vel_mf_joint_nb", "phase_nb", "phase_poisson"])
def test_sampled_counts_are_calibrated_and_a_wrong_dispersion_is_not(case):
    z = _resampled(case, 3)
    e = Q.evaluate(z, SEED)
    for m, v in e.items():
        gene, _ = Q.histograms(v["u"].numpy(), 20)
        _, zg, _ = Q.uniformity(gene)
        _, zp, edge = Q.uniformity(gene.sum(0))
        print(f"{case} {m}: pooled z {zp:.2f}, worst gene z {zg.max():.2f}, edge share {edge:.3f}")
        assert zp < Q.GOF_Z and zg.max() < Q.GOF_Z, (case, m, zp, zg.max())
    if "draw_shape_inv" in z:
        z["draw_shape_inv"] = z["draw_shape_inv"] / 8
        for m, v in Q.evaluate(z, SEED).items():
            _, zp, edge = Q.uniformity(Q.histograms(v["u"].numpy(), 20)[0].sum(0))
            print(f"{case} {m} scored with shape_inv / 8: pooled z {zp:.1f}, edge share {edge:.3f}")
            assert zp > 60 and edge > 0.15, (case, m, zp, edge)


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
        predictive.predictive_pit(_fake_engine("Lognormal"), draws, seed=1)
    for bad in (1, 65, 0, -3):
        with pytest.raises(ValueError, match="bins must lie in"):
            predictive.predictive_pit(_fake_engine(), draws, seed=1, bins=bad)
    with pytest.raises(ValueError, match="'ν' and 'ϕxy'"):
        predictive.predictive_pit(_fake_engine(), {"ν": draws["ν"]}, seed=1)
    big = _fake_engine()
    big.spec.Ng, big.Nc_local = 10000, 10000                  # 2 x 12 x 1e8 bytes > 2^30, while 2 x 4 x 1e8 would pass
    assert 4 * 2 * 10 ** 8 < predictive.MAX_POINTWISE_BYTES < 12 * 2 * 10 ** 8
    with pytest.raises(ValueError, match="return_pointwise"):
        predictive.predictive_pit(big, {"ν": torch.zeros(1, 1, 1), "ϕxy": torch.zeros(1, 1, 2)}, seed=1, return_pointwise=True)
    mp = types.SimpleNamespace(model_fn=None, guide_fn=None)
    for cls in (PhaseFitModel, VelocityFitModel):
        with pytest.raises(ValueError, match="not been fitted"):
            cls(mp).predictive_pit()
        f = cls(mp)
        f.engine, f.losses, f.spec = _fake_engine("Lognormal"), [1.0], _fake_engine("Lognormal").spec
        with pytest.raises(NotImplementedError, match="Lognormal"):
            f.predictive_pit()
        f.engine, f.spec = _fake_engine(), _fake_engine().spec
        with pytest.raises(ValueError, match="bins must lie in"):
            f.predictive_pit(bins=100)
        with pytest.raises(ValueError, match="at least 1 draw"):
            f.predictive_pit(num_samples=0)


def test_header_declares_and_lib_binds_vc_predictive_pit():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    m = re.search(r"\bint vc_predictive_pit\(vc_engine\* e, int64_t n_draws,([^;]*)\);", hdr)
    assert m, "vc_predictive_pit is not declared"
    arity = 2 + m.group(1).count(",") + 1
    assert "vc_predictive_pit" in _lib.EXPORTS and len(_lib.EXPORTS["vc_predictive_pit"][1]) == arity == 22
    assert "#define VC_ABI_VERSION 2" in hdr and _lib.VC_ABI_VERSION == 2
    # the draw arguments are those of its two neighbours, in their order
    pw, pit = _lib.EXPORTS["vc_pointwise_density"][1], _lib.EXPORTS["vc_predictive_pit"][1]
    assert pit[:14] == pw[:14] and pit[14:16] == [C.c_uint64, C.c_int32]
    assert "uint64_t seed, int32_t n_bins" in m.group(1) and "stage 2" in hdr and "non-integer counts" in hdr


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)                    # never dereferenced: every call below is refused before anything is launched

    def call(e, n_draws=4, bins=20, gene=one, cell=one, phixy=one):
        return lib.vc_predictive_pit(e, n_draws, phixy, 0, one, 0, None, one, None, 0, None, 0, None, 0, 7, bins, 0, 8, gene, cell, None, None)
    assert call(None) == _lib.VC_ERR_ARG and b"null engine" in lib.vc_last_error(None)
    cfg = _lib.vc_config(abi_version=_lib.VC_ABI_VERSION, model=0, guide=0, noise=0, with_delta_nu=0, n_harmonics=1, n_harmonics_w=0,
                         Nb=1, Nx=0, lrmn_rank=5, rank=0, world_size=1, Ng=5, Nc_local=8, Nc_global=8, cell_offset=0, gamma_alpha=1.0,
                         gamma_beta=2.0, sigma_ln_s=0.5, sigma_ln_u=0.1, rho_mean=4.0, rho_std=1.0, rho_scale=1.0)
    h = C.c_void_p()
    assert lib.vc_create(C.byref(cfg), C.byref(h)) == _lib.VC_OK
    try:
        assert call(h, n_draws=0) == _lib.VC_ERR_ARG and b"n_draws must be >= 1" in lib.vc_last_error(h)
        assert call(h, n_draws=(1 << 20) + 1) == _lib.VC_ERR_ARG and b"2^20" in lib.vc_last_error(h)
        for bad in (1, 65, 0, -1):
            assert call(h, bins=bad) == _lib.VC_ERR_ARG and b"n_bins must lie in [2, 64]" in lib.vc_last_error(h)
        assert call(h, gene=None) == _lib.VC_ERR_ARG and b"null gene_hist_dev" in lib.vc_last_error(h)
        assert call(h, cell=None) == _lib.VC_ERR_ARG
        assert call(h) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
        # the entry point's own refusals come before the ones it shares with its neighbours (null phixy), in their order
        assert call(h, n_draws=0, phixy=None) == _lib.VC_ERR_ARG and b"n_draws must be >= 1" in lib.vc_last_error(h)
        assert call(h, bins=1, gene=None) == _lib.VC_ERR_ARG and b"n_bins" in lib.vc_last_error(h)
        assert call(h, phixy=None) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
    finally:
        lib.vc_destroy(h)


def _record(gene, cell, pw=None, **kw):
    from velocycle_amd.predictive import PredictivePIT
    args = dict(n_draws=3, bins=4, seed=9)
    args.update(kw)
    return PredictivePIT(gene_hist={"S": torch.tensor(gene, dtype=torch.int64)}, cell_hist={"S": torch.tensor(cell, dtype=torch.int64)},
                         pointwise=None if pw is None else {"S": torch.tensor(pw, dtype=torch.float32)}, **args)


def test_merge_pit_shards_on_hand_made_records():
    from velocycle_amd.predictive import merge_pit_shards
    big = 2 ** 53 + 1                                        # an integer float64 cannot hold: the gene tables are added as integers
    a = _record([[1, 0, 2, 0], [big, 0, 0, 0]], [[1, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0]], pw=np.arange(18).reshape(3, 2, 3))
    b = _record([[0, 1, 0, 0], [1, 0, 0, 1]], [[0, 1, 0, 1]], pw=100 + np.arange(6).reshape(3, 2, 1))
    got = merge_pit_shards([a, b])
    assert got.gene_hist["S"].tolist() == [[1, 1, 2, 0], [big + 1, 0, 0, 1]] and got.gene_hist["S"].dtype == torch.int64
    assert got.cell_hist["S"].tolist() == [[1, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 1]]
    assert got.pointwise["S"].shape == (3, 2, 4) and got.pointwise["S"][1, 0].tolist() == [6.0, 7.0, 8.0, 102.0]
    assert (got.n_draws, got.bins, got.seed) == (3, 4, 9)
    assert merge_pit_shards([a]).gene_hist["S"].tolist() == a.gene_hist["S"].tolist()
    for kw in (dict(seed=8), dict(bins=5), dict(n_draws=2)):
        with pytest.raises(ValueError, match="different draws, seeds or bins"):
            merge_pit_shards([a, _record([[0, 1, 0, 0], [1, 0, 0, 1]], [[0, 1, 0, 1]], pw=np.zeros((3, 2, 1)), **kw)])
    with pytest.raises(ValueError, match="only some"):
        merge_pit_shards([a, _record([[0, 1, 0, 0], [1, 0, 0, 1]], [[0, 1, 0, 1]])])


def test_summary_arithmetic():
    rec = _record([[5, 5, 5, 5], [20, 0, 0, 0], [4, 1, 1, 4]], [[10, 2, 2, 6], [19, 4, 4, 3]])
    g = rec.gene()["S"]
    # chi2 = sum (h - n / B)^2 / (n / B);  z = (chi2 - (B - 1)) / sqrt(2 (B - 1));  edge share = (first + last) / n
    assert g["chi2"].tolist() == pytest.approx([0.0, 60.0, (1.5 ** 2 * 4) / 2.5])
    assert g["z"].tolist() == pytest.approx([-3 / np.sqrt(6), 57 / np.sqrt(6), (3.6 - 3) / np.sqrt(6)])
    assert g["edge_share"].tolist() == pytest.approx([0.5, 1.0, 0.8]) and g["z"].dtype == torch.float64
    c = rec.cell()["S"]
    assert c["chi2"].tolist() == pytest.approx([(25 + 9 + 9 + 1) / 5.0, (11.5 ** 2 + 3.5 ** 2 * 2 + 4.5 ** 2) / 7.5])
    p = rec.pooled()["S"]
    assert p["hist"].tolist() == [29, 6, 6, 9] and p["chi2"] == pytest.approx((16.5 ** 2 + 6.5 ** 2 * 2 + 3.5 ** 2) / 12.5)
    assert p["edge_share"] == pytest.approx(38 / 50) and p["z"] == pytest.approx((p["chi2"] - 3) / np.sqrt(6))
    chi2, z, edge = Q.uniformity(rec.gene_hist["S"].numpy())              # the checker's own arithmetic agrees
    assert np.allclose(chi2, g["chi2"].numpy()) and np.allclose(z, g["z"].numpy()) and np.allclose(edge, g["edge_share"].numpy())


def test_checker_histograms_and_uniforms():
    u = np.array([[0.0, 0.049999, 0.05, 0.999999, 0.5], [0.95, 0.2, 0.2, 0.2, 0.0]])
    gene, cell = Q.histograms(u, 20)
    assert gene.sum(1).tolist() == [5, 5] and cell.sum(1).tolist() == [2] * 5
    assert gene[0, 0] == 2 and gene[0, 1] == 1 and gene[0, 19] == 1 and gene[0, 10] == 1 and gene[1, 4] == 3 and gene[1, 19] == 1
    assert Q.bins_of(np.array([1.0]), 7).tolist() == [6]                  # the clamp of the last bin
    # v: exact in float32, a function of (seed, matrix, gene, GLOBAL cell) alone
    v = Q.uniforms(3, 10, 5, 0)
    assert np.array_equal(v, Q.uniforms(3, 10, 5, 0, dt=np.float32).astype(np.float64)) and bool(((v > 0) & (v < 1)).all())
    assert np.array_equal(Q.uniforms(3, 4, 5, 0, cell_offset=6), v[:, 6:]) and not np.array_equal(Q.uniforms(3, 10, 5, 1), v)
    assert not np.array_equal(Q.uniforms(3, 10, 6, 0), v)
    near = Q.near_edge(np.array([0.05 + 1e-9, 0.07, 1e-9, 1 - 1e-9]), np.full(4, 1e-7), 20)
    assert near.tolist() == [True, False, False, False]


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_pit_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly emitted for gfx950
    (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_pit.hip")
    out = str(tmp_path / "pit.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.name:\s+(\S*vc_pit_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", txt)
    assert len(found) == 24, len(found)                    # H 1..3 x {phase, velocity} x {NB, Poisson} x {u16, f32}
    assert all(int(n) == 0 for _, n in found), [f for f in found if int(f[1])]


def test_counts_the_kernel_cannot_count_down_from_are_refused_on_the_host(tmp_path):
    """vc_pit_count_ok of csrc/vc_host_logic.h, the predicate vc_predictive_pit refuses an engine by before any launch, in a small
    program of its own: integers in [0, 2^24) pass; fractions, negatives, 2^24 and beyond (where float32's k - 1 can round back to
    k and a float countdown would never end), infinities and NaN do not."""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    src = tmp_path / "pit_count.cpp"
    src.write_text('''#include <cmath>
#include <cstdio>
#include <limits>
#include "vc_host_logic.h"
int main() {
  const float ok[] = {0.f, 1.f, 255.f, 60000.f, 65536.f, 16777215.f};
  const float bad[] = {0.5f, 1.25f, -1.f, 16777216.f, 16777220.f, 33554432.f, 3.0e38f, std::numeric_limits<float>::infinity(),
                       -std::numeric_limits<float>::infinity(), std::nanf("")};
  int wrong = 0;
  for (float v : ok) if (!vc_pit_count_ok(v)) { std::printf("refused %g\\n", (double)v); ++wrong; }
  for (float v : bad) if (vc_pit_count_ok(v)) { std::printf("accepted %g\\n", (double)v); ++wrong; }
  // every admitted count can be counted down in float32: k - 1 is a different, exact float
  for (float v : ok) if (v >= 1.f && !(v - 1.f < v && (double)(v - 1.f) == (double)v - 1.0)) { std::printf("countdown %g\\n", (double)v); ++wrong; }
  const float t = 16777220.f;
  if (16777216.f + 1.f != 16777216.f || t - 1.f != t) { std::printf("float32 counts on past 2^24?\\n"); ++wrong; }
  return wrong;
}
''')
    exe = str(tmp_path / "pit_count")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "velocycle_amd", "csrc"), str(src), "-o", exe], check=True,
                   capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    eng = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_engine.hip")).read()
    body = eng[eng.index('extern "C" int vc_predictive_pit'):]
    assert body.index("vc_pit_count_ok") < body.index("vc_launch_pit") and body.index("vc_pit_count_ok") < body.index("pw_tables(e)")
    assert "2^24" in open(os.path.join(ROOT, "include", "velocycle_hip.h")).read().split("int vc_predictive_pit(")[0].split("predictive PIT")[-1]
