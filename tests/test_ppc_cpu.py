"""CPU: the numpy restatement of the device count sampler (tests/ppc_checker.py) against the exact pmfs of torch.distributions
(moments and a chi-square on near-equiprobable bins, over rates up to the documented 2^20); the float32 restatement's own share of differing elements (what caps the device in tests/test_hip_ppc.py); the refusals of the public
face before any library call; merge_check_shards; the C ABI declarations and bindings; the code object's private segment."""
import os
import re
import subprocess
import types
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import ppc_checker as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N_CELL = 20240917, 1 << 16          # Philox key and samples per grid cell of the CPU run
N_LARGE = 1 << 18                         # samples per cell of LARGE_GRID (CPU and device)


def test_philox_matches_the_published_vectors():
    # Random123 known-answer tests of philox4x32-10
    assert [int(x) for x in K.philox(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(x) for x in K.philox(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(x) for x in K.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_grid_exercises_every_branch():
    mus = [m for m, r in K.GRID if r is None]
    assert min(mus) < 0.1 and any(m < K.SMALL for m in mus) and any(K.SMALL < m < 12 for m in mus) and max(mus) >= 300
    rs = [r for _, r in K.GRID if r is not None]
    assert any(r < 1 for r in rs) and any(r == 1 for r in rs) and any(r > 1 for r in rs)
    assert any(r is not None and m > 100 for m, r in K.GRID) and any(r is not None and m < 0.1 for m, r in K.GRID)
    # the large grid: Poisson rates on both sides of 2^16 (counts past uint16) and up to the documented range, NB at large means
    big = [m for m, r in K.LARGE_GRID if r is None]
    assert any(m < 65536 for m in big) and any(m > 65536 for m in big) and all(m <= K.MU_MAX for m, _ in K.LARGE_GRID)
    assert any(m >= 0.9 * K.MU_MAX for m in big)
    assert any(r is not None and m >= 1e5 for m, r in K.LARGE_GRID)
    # the gamma mixing leaves (almost) every rate of the NB cells inside the range: refusals are test_sampler_range_is_refused_...'s
    n = 1 << 16
    idx = np.arange(n, dtype=np.uint64)
    for mu, r in K.LARGE_GRID:
        if r is not None:
            g = K.gamma(SEED, idx, 0, 1, np.full(n, r), np.float64)
            assert (g > 0).all() and float((g * K.handed_rate(mu) / r > K.MU_MAX).mean()) < 1e-4, (mu, r)


def fmt_z(z):
    return f"|z| mean {z['mean']:.2f} variance {z['var']:.2f} zero share {z['zero']:.2f} chi-square {z['gof']:+.2f}"


def test_gof_z_is_centred_on_exact_samples_and_sees_a_shifted_rate():
    """gof_z against numpy's own samplers: near 0 on samples of the distribution itself (bins merged at small rates), far out for a
    rate 1 % off at 2^16 samples (mu = 1e4: a shift of one standard deviation)."""
    rng = np.random.default_rng(5)
    n = 1 << 16
    for mu, r in ((0.02, None), (3.0, None), (300.0, None), (1.0e4, None), (12.0, 0.7), (1.0e4, 2.0)):
        k = rng.poisson(mu, n) if r is None else rng.poisson(rng.gamma(r, mu / r, n))
        assert abs(K.gof_z(k, mu, r)) <= 3.5, (mu, r)
    assert K.gof_z(rng.poisson(1.01e4, n), 1.0e4, None) > 100.0
    assert K.gof_z(rng.poisson(rng.gamma(2.0, 5.0e3, n)), 1.0e4, 2.5) > 20.0


def test_restated_sampler_against_exact_pmfs():
    k64 = K.sample_grid(N_CELL, SEED, 0, np.float64)
    assert (k64 >= 0).all()
    worst = 0.0
    for i, (mu, r) in enumerate(K.GRID):
        z = K.moment_z(k64[i * N_CELL:(i + 1) * N_CELL], K.exact_moments(mu, r))
        print(f"mu {mu} r {r}: |z| mean {z['mean']:.2f} variance {z['var']:.2f} zero share {z['zero']:.2f}")
        worst = max(worst, *z.values())
        assert all(v <= 6.0 for v in z.values()), (mu, r, z)
    # another draw and another matrix are other streams
    again = K.sample_grid(4096, SEED, 1, np.float64)
    assert (again != k64.reshape(len(K.GRID), N_CELL)[:, :4096].reshape(-1)).mean() > 0.3


GRIDS = {"grid": K.GRID, "large": K.LARGE_GRID}


@lru_cache(maxsize=None)
def restated(which, dtype_name):
    """The restated sampler over GRIDS[which] at N_LARGE samples per cell, seed SEED, draw 0, with the r the device forms: computed
    once, shared by the CPU tests and the device tests (tests/test_hip_ppc.py), never written to."""
    k = K.sample_grid(N_LARGE, SEED, 0, getattr(np, dtype_name), GRIDS[which], as_device=True)
    k.setflags(write=False)
    return k


def exact_cell(which, i):
    """(mu, r) the exact distribution of cell i is taken at: the rate exp(float64(float32(log mu))) the sampler is handed (for GRID
    the grid's own mu, as every test of it does) and the r the device forms."""
    mu, r = GRIDS[which][i]
    return (K.handed_rate(mu) if which == "large" else mu), (None if r is None else float(K.device_r(r)))


def assert_cells_within_bars(which):
    """Both restatements over a grid at N_LARGE samples per cell: no count is -1, every |z| and the chi-square <= 6.0, the float64
    restatement's <= 3.5."""
    n, bad = N_LARGE, []
    for i, (mu, r) in enumerate(GRIDS[which]):
        for dt, bar in (("float64", 3.5), ("float32", 6.0)):
            kk = restated(which, dt)[i * n:(i + 1) * n]
            assert (kk >= 0).all(), (mu, r, dt)
            z = K.cell_z(kk, *exact_cell(which, i))
            print(f"mu {mu:g} r {r} {dt}: {fmt_z(z)}")
            if not all(v <= bar for v in z.values()):
                bad.append((mu, r, dt, {name: round(float(v), 2) for name, v in z.items()}))
    assert not bad, bad


def test_chi_square_of_both_restatements_over_the_grid():
    """gof_z (and the moments once more) over GRID, at the 2^18 samples per cell and the seed of the device test, so that the
    figures printed here stand next to the device's.  The float64 restatement is <= 3.5: the seed condition.  (The 2^16 samples of
    test_restated_sampler_against_exact_pmfs do not meet it: by chance their zero share at mu = 0.02 is 3.2 standard errors out,
    which on that cell's two bins, one degree of freedom, is the same number squared: a chi-square of +6.6.)"""
    assert_cells_within_bars("grid")


def test_restated_sampler_against_exact_pmfs_up_to_the_documented_range():
    """Both restatements over LARGE_GRID (Poisson 1e3 .. 1e6, NB means 1e4 .. 2e5) at 2^18 samples per cell (about 10 s of numpy),
    against the exact moments and pmf at the rate the sampler is handed, exp(float64(float32(log mu))).  Every |z| and the
    standardised chi-square are <= 6.0, the float64 restatement's <= 3.5 (a condition on the seed: it is not near the bar by
    chance), no count is -1.  With PTRS's full test in float32 (k ln lam - lam and ln k! cancel from ~1.4e7 down to a log-probability
    of order -1 .. -10) the float32 restatement fails this test on the Poisson cells from 1e5 on: chi-square +9.8 at 1e5, variance |z| 16.7 and
    chi-square +54.6 at 5e5, 7.6 and +51.7 at 1e6."""
    assert_cells_within_bars("large")


def test_float32_restatement_differs_in_a_small_non_zero_share():
    n = 1 << 16
    a, b = K.sample_grid(n, SEED, 0, np.float64), K.sample_grid(n, SEED, 0, np.float32)
    share = float((a != b).mean())
    print(f"float32 against float64 restatement: {int((a != b).sum())} of {a.size} elements differ (share {share:.2e})")
    assert (b >= 0).all() and 0 < share < 2e-4
    assert K.cap(0, a.size) == K.FLOOR and K.cap(100, a.size) == 400


def test_sampler_range_is_refused_not_made_up():
    eta = np.log(np.array([2.0e6, 1.0e6, np.inf, 5.0], dtype=np.float32))
    for dt in (np.float64, np.float32):
        k = K.sample_counts(eta, None, 1, 0, 0, np.arange(4, dtype=np.uint64), dt)
        assert k[0] == K.FAIL and k[1] > 0 and k[2] == K.FAIL and k[3] >= 0
        k = K.sample_counts(eta[3:], np.array([0.0]), 1, 0, 0, np.arange(1, dtype=np.uint64), dt)
        assert k[0] == K.FAIL


def _fake_engine(noise="NegativeBinomial", kind="velocity", generic=0):
    spec = types.SimpleNamespace(kind=kind, noisemodel=noise, Ng=5, Nc=8, H=1, Hw=1, Nh=3, Nhw=3, Nb=1, Nx=1, with_delta_nu=False,
                                 condition_on={})
    return types.SimpleNamespace(spec=spec, Nc_local=8, stats={"generic": generic})


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
        predictive.predictive_check(_fake_engine("Lognormal"), draws, seed=1)
    with pytest.raises(NotImplementedError, match="run-time-sized"):
        predictive.predictive_check(_fake_engine(generic=1), draws, seed=1)
    with pytest.raises(ValueError, match="at least 1 draw"):
        predictive.predictive_check(_fake_engine(), {k: v[:0] for k, v in draws.items()}, seed=1)
    with pytest.raises(ValueError, match="keep_replicates must lie"):
        predictive.predictive_check(_fake_engine(), draws, seed=1, keep_replicates=5)
    big = _fake_engine()
    big.spec.Ng, big.Nc_local = 40000, 40000
    with pytest.raises(ValueError, match="dense replicates"):
        predictive.predictive_check(big, {"ν": torch.zeros(2, 1, 1), "ϕxy": torch.zeros(2, 1, 2)}, seed=1, keep_replicates=1)
    mp = types.SimpleNamespace(model_fn=None, guide_fn=None)
    for cls in (PhaseFitModel, VelocityFitModel):
        with pytest.raises(ValueError, match="not been fitted"):
            cls(mp).posterior_predictive_check()
        f = cls(mp)
        f.engine, f.losses, f.spec = _fake_engine("Lognormal"), [1.0], _fake_engine("Lognormal").spec
        with pytest.raises(NotImplementedError, match="Lognormal"):
            f.posterior_predictive_check()
        f.engine, f.spec = _fake_engine(), _fake_engine().spec
        with pytest.raises(ValueError, match="at least 1 draw"):
            f.posterior_predictive_check(num_samples=0)
    with pytest.raises(ValueError, match="device tensor"):
        predictive.sample_counts(torch.zeros(4), seed=1)


def _record(rng, D, Ng, Nc, mats=("S", "U"), keep=0, seed=3):
    from velocycle_amd.predictive import PredictiveCheck
    rep = {m: rng.integers(0, 1 << 40, size=(D, Ng, Nc)) % rng.integers(1, 5000, size=(1, Ng, 1)) for m in mats}
    obs = {m: rng.integers(0, 3000, size=(Ng, Nc)) for m in mats}
    t = lambda x, dt: torch.tensor(np.ascontiguousarray(x), dtype=dt)
    gene_rep = {m: t(K.rep_stats(rep[m])[0], torch.int64) for m in mats}
    cell_rep = {m: t(K.rep_stats(rep[m])[1], torch.int64) for m in mats}
    gene_obs = {m: t(K.obs_stats(obs[m])[0], torch.float64) for m in mats}
    cell_obs = {m: t(K.obs_stats(obs[m])[1], torch.float64) for m in mats}
    reps = {m: t(rep[m][:keep], torch.int32) for m in mats} if keep else None
    return PredictiveCheck(gene_rep, cell_rep, gene_obs, cell_obs, D, Nc, seed, reps), rep, obs


def test_merge_check_shards_is_exact_and_the_derived_values_follow_their_definitions():
    from velocycle_amd.predictive import PredictiveCheck, STATISTICS, merge_check_shards
    rng = np.random.default_rng(11)
    D, Ng, Nc = 7, 9, 23
    whole, rep, obs = _record(rng, D, Ng, Nc, keep=2)
    cuts = [(0, 5), (5, 6), (6, 23)]
    parts = []
    for a, b in cuts:
        t = lambda x, dt: torch.tensor(np.ascontiguousarray(x), dtype=dt)
        parts.append(PredictiveCheck({m: t(K.rep_stats(rep[m][:, :, a:b])[0], torch.int64) for m in rep},
                                     {m: t(K.rep_stats(rep[m][:, :, a:b])[1], torch.int64) for m in rep},
                                     {m: t(K.obs_stats(obs[m][:, a:b])[0], torch.float64) for m in rep},
                                     {m: t(K.obs_stats(obs[m][:, a:b])[1], torch.float64) for m in rep}, D, b - a, 3,
                                     {m: t(rep[m][:2, :, a:b], torch.int32) for m in rep}))
    got = merge_check_shards(parts)
    assert got.n_cells == Nc and got.n_draws == D
    for f in ("gene_rep", "cell_rep", "gene_obs", "cell_obs", "replicates"):
        for m in ("S", "U"):
            assert torch.equal(getattr(got, f)[m], getattr(whole, f)[m]), (f, m)
    parts[1].seed = 4
    with pytest.raises(ValueError, match="different draws or seeds"):
        merge_check_shards(parts)
    # derived values against the checker's own formulas
    T_rep = K.derived(whole.gene_rep["S"].numpy(), Nc)
    T_obs = K.derived(whole.gene_obs["S"].numpy(), Nc)
    assert np.array_equal(whole.gene_T_rep["S"].numpy(), T_rep) and np.array_equal(whole.gene_T_obs["S"].numpy(), T_obs)
    assert np.allclose(T_rep[:, 1], rep["S"].astype(np.float64).var(2), rtol=1e-9)
    for j, s in enumerate(STATISTICS):
        ge, gt, mid = K.p_values(T_rep[:, j], T_obs[j])
        g = whole.gene(s)["S"]
        assert np.array_equal(g["p_ge"].numpy(), ge) and np.array_equal(g["p_gt"].numpy(), gt) and np.array_equal(g["p_mid"].numpy(), mid)
        assert np.allclose(g["rep_mean"].numpy(), T_rep[:, j].mean(0)) and np.allclose(g["rep_sd"].numpy(), T_rep[:, j].std(0, ddof=1))
    lib = whole.library_size()["U"]
    ge, gt, mid = K.p_values(rep["U"].sum(1).astype(np.float64), obs["U"].sum(0).astype(np.float64))
    assert np.array_equal(lib["p_ge"].numpy(), ge) and np.array_equal(lib["p_mid"].numpy(), mid) and lib["obs"].shape == (Nc,)


def test_header_declares_and_lib_binds_both_entry_points():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    for name, first, arity in (("vc_sample_counts", r"const float\* eta_dev", 11), ("vc_predictive_check", r"vc_engine\* e", 26)):
        m = re.search(r"\bint " + name + r"\(" + first + r",([^;]*)\);", hdr)
        assert m, f"{name} is not declared"
        assert 1 + m.group(1).count(",") + 1 == arity == len(_lib.EXPORTS[name][1]), name
    assert "#define VC_ABI_VERSION 2" in hdr and _lib.VC_ABI_VERSION == 2
    assert "#define VC_ERR_RANGE (-6)" in hdr and _lib.VC_ERR_RANGE == -6
    assert "velocity_inference_model.py:385-386" in hdr and "GammaPoisson" in hdr


def test_entry_points_validate_without_a_device():
    import ctypes as C
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)                    # never dereferenced: every call below is refused before anything is launched
    assert lib.vc_sample_counts(None, 1, 1, None, 1, 0, 0, 0, 1, one, None) == _lib.VC_ERR_ARG and b"null eta_dev" in lib.vc_last_error(None)
    assert lib.vc_sample_counts(one, 0, 1, None, 1, 0, 0, 0, 1, one, None) == _lib.VC_ERR_ARG
    assert lib.vc_sample_counts(one, 1, 1, None, 1, -1, 0, 0, 1, one, None) == _lib.VC_ERR_ARG and b"draw" in lib.vc_last_error(None)
    assert lib.vc_sample_counts(one, 1, 1, None, 1, 0, 1 << 16, 0, 1, one, None) == _lib.VC_ERR_ARG

    def call(e, n_draws=4, gene=one, cell=one, d0=0, nd=4, phixy=one):
        return lib.vc_predictive_check(e, n_draws, phixy, 0, one, 0, None, one, None, 0, None, 0, None, 0, 7, 0, 8, d0, nd, gene, cell, None, None,
                                       None, 0, None)
    assert call(None) == _lib.VC_ERR_ARG and b"null engine" in lib.vc_last_error(None)
    cfg = _lib.vc_config(abi_version=_lib.VC_ABI_VERSION, model=0, guide=0, noise=0, with_delta_nu=0, n_harmonics=1, n_harmonics_w=0,
                         Nb=1, Nx=0, lrmn_rank=5, rank=0, world_size=1, Ng=5, Nc_local=8, Nc_global=8, cell_offset=0, gamma_alpha=1.0,
                         gamma_beta=2.0, sigma_ln_s=0.5, sigma_ln_u=0.1, rho_mean=4.0, rho_std=1.0, rho_scale=1.0)
    h = C.c_void_p()
    assert lib.vc_create(C.byref(cfg), C.byref(h)) == _lib.VC_OK
    try:
        assert call(h, n_draws=0) == _lib.VC_ERR_ARG and b"n_draws" in lib.vc_last_error(h)
        assert call(h, gene=None) == _lib.VC_ERR_ARG and b"null gene_rep_dev" in lib.vc_last_error(h)
        assert call(h, cell=None) == _lib.VC_ERR_ARG
        assert call(h) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
        # a call that one of the refusals shared with vc_pointwise_density would stop too (null phixy) still meets the entry point's
        # own refusals first, in their order
        assert call(h, n_draws=0, phixy=None) == _lib.VC_ERR_ARG and b"n_draws must be >= 1" in lib.vc_last_error(h)
        assert call(h, gene=None, phixy=None) == _lib.VC_ERR_ARG and b"null gene_rep_dev" in lib.vc_last_error(h)
        assert call(h, phixy=None) == _lib.VC_ERR_STATE and b"before vc_finalize" in lib.vc_last_error(h)
    finally:
        lib.vc_destroy(h)


def test_new_kernels_have_no_scratch(tmp_path):
    """Every instantiation of the kernels of vc_ppc.hip reports .private_segment_fixed_size 0 in the metadata of the assembly emitted
    for gfx950 (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_ppc.hip")
    out = str(tmp_path / "ppc.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.name:\s+(\S*(?:vc_ppc_kernel|vc_ppc_observed_\w+_kernel|vc_sample_counts_kernel)\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", txt)
    names = [n for n, _ in found]
    assert sum("vc_ppc_kernel" in n for n in names) == 12          # H 1..3 x {phase, velocity} x {NB, Poisson}
    assert sum("vc_sample_counts_kernel" in n for n in names) == 2 and sum("vc_ppc_observed" in n for n in names) == 4
    assert all(int(n) == 0 for _, n in found), [f for f in found if int(f[1])]
