"""GPU: the device count sampler (vc_sample_counts) and the posterior predictive check (vc_predictive_check) against the float64
checker (tests/ppc_checker.py).  Counts are compared for EQUALITY; a float32 evaluation may land on the other side of an accept /
floor / search decision, so a share of elements may differ: at most SAFETY (4) x the number the float32 restatement itself differs
from the float64 one in on the same inputs, at least 16 elements.  Statistics are compared exactly.  Against the exact pmf (moments
and the chi-square gof_z) the sampler is held over rates up to its documented 2^20, and the 64-bit statistics at counts past 2^16."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import ppc_checker as K
from tests.test_hip_pointwise import cut, draws_of, engine_of
from tests.test_pointwise_cpu import CASES, load
from tests.test_ppc_cpu import GRIDS, N_LARGE, SEED, exact_cell, fmt_z, restated

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_CELL = N_LARGE                      # samples per grid cell, 2^18: 16 cells = 2^22 elements
TABLES = ("gene_rep", "cell_rep", "gene_obs", "cell_obs")


def device_grid(n, seed, draw, grid=None):
    """vc_sample_counts over a grid (ppc_checker.GRID unless given) in the layout of ppc_checker.sample_grid."""
    from velocycle_amd.predictive import sample_counts
    grid = K.GRID if grid is None else grid
    eta, r = K.grid_inputs(n, grid)
    n_p = sum(1 for _, rr in grid if rr is None)
    assert all(rr is None for _, rr in grid[:n_p]) and all(rr is not None for _, rr in grid[n_p:])
    e = torch.tensor(eta, device=DEV)
    kp = sample_counts(e[:n_p * n], seed=seed, draw=draw, matrix=0, index_origin=0)
    si = torch.tensor([1.0 / np.float32(rr) for _, rr in grid[n_p:]], dtype=torch.float32)
    kn = sample_counts(e[n_p * n:].reshape(-1, n), si, seed=seed, draw=draw, matrix=1, index_origin=n_p * n, row_index_stride=n)
    # the shared restatements (tests/test_ppc_cpu.py: restated) divide by the same float32 r = 1 / shape_inv the device forms
    assert [float(np.float32(1.0) / x) for x in si.numpy()] == [float(K.device_r(rr)) for _, rr in grid[n_p:]]
    return torch.cat([kp, kn.reshape(-1)]).cpu().numpy().astype(np.int64)


def test_sampler_against_the_float64_checker_and_the_exact_moments():
    got = device_grid(N_CELL, SEED, 0)
    assert got.size >= 1 << 22 and (got >= 0).all()
    k64, k32 = restated("grid", "float64"), restated("grid", "float32")
    d32, dgpu = int((k32 != k64).sum()), int((got != k64).sum())
    print(f"\n[sampler, {got.size} elements] float32 restatement differs from float64 in {d32} (share {d32 / got.size:.2e}), "
          f"device in {dgpu} (share {dgpu / got.size:.2e}); cap {K.cap(d32, got.size)}")
    for i, (mu, r) in enumerate(K.GRID):
        sl = slice(i * N_CELL, (i + 1) * N_CELL)
        z = K.moment_z(got[sl], K.exact_moments(mu, r))
        gof = K.gof_z(got[sl], mu, r)
        print(f"  mu {mu} r {r}: device |z| mean {z['mean']:.2f} variance {z['var']:.2f} zero share {z['zero']:.2f} chi-square {gof:+.2f}; "
              f"differing float32 {int((k32[sl] != k64[sl]).sum())} device {int((got[sl] != k64[sl]).sum())}")
        assert all(v <= 6.0 for v in z.values()), (mu, r, z)
        assert gof <= 6.0, (mu, r, gof)
    assert 0 < d32 < 1e-3 * got.size
    assert dgpu <= K.cap(d32, got.size), (dgpu, d32)


def test_sampler_against_the_exact_pmf_up_to_the_documented_range():
    """vc_sample_counts over LARGE_GRID (Poisson 1e3 .. 1e6, NB means 1e4 .. 2e5; 2^18 samples per cell): no element is -1, and the
    moments' |z| and the chi-square against the exact pmf at the rate the sampler is handed are <= 6.0.

    The share of elements that differ from the float64 checker is PRINTED for the device and for the float32 restatement and NOT
    held to the 4 x cap of the other tests, on purpose: at these rates mu = 2^(eta log2 e) itself moves by up to ~1e-6 relative
    with the float32 rounding of eta log2 e, about +-1 at 1e6, and with it about half of the counts.  Elementwise equality says
    nothing about the kernel there; the distribution does.  Do not add the cap."""
    got = device_grid(N_LARGE, SEED, 0, K.LARGE_GRID)
    assert got.size == len(K.LARGE_GRID) * N_LARGE and (got >= 0).all()
    k64, k32 = restated("large", "float64"), restated("large", "float32")
    bad = []
    print()
    for i, (mu, r) in enumerate(K.LARGE_GRID):
        sl = slice(i * N_LARGE, (i + 1) * N_LARGE)
        z = K.cell_z(got[sl], *exact_cell("large", i))
        print(f"  mu {mu:g} r {r}: device {fmt_z(z)}; share differing from float64: float32 restatement "
              f"{float((k32[sl] != k64[sl]).mean()):.2e}, device {float((got[sl] != k64[sl]).mean()):.2e}")
        if not all(v <= 6.0 for v in z.values()):
            bad.append((mu, r, {name: round(float(v), 2) for name, v in z.items()}))
    assert not bad, bad


def test_sampler_edges():
    """Rate 0 (eta = -200 underflows, eta = -inf), the top of the range, nan, and the negative binomial at its two ends: r = 1e6
    (a Poisson in all but name; the gamma's d = r - 1/3 is large) and r = 0.02 (deep in the boost g u^(1/r); almost all zeros)."""
    from velocycle_amd import _lib
    from velocycle_amd.predictive import sample_counts
    zero = torch.tensor([-200.0, -math.inf] * 500, device=DEV)
    assert int(sample_counts(zero, seed=SEED).abs().max()) == 0
    assert int(sample_counts(zero.reshape(2, 500), torch.tensor([0.5, 4.0]), seed=SEED, matrix=1).abs().max()) == 0
    top = sample_counts(torch.full((1000,), math.log(2.0 ** 20), device=DEV), seed=SEED)
    assert bool((top > 2 ** 20 - 8 * 1024).all()) and bool((top < 2 ** 20 + 8 * 1024).all())        # +-8 sd, sd = 2^10
    with pytest.raises(_lib.CountSamplerRangeError):
        sample_counts(torch.tensor([1.0, math.nan, 2.0], device=DEV), seed=SEED)
    n = N_LARGE
    cells = [(5.0, 1.0e-6), (50.0, 1.0e-6), (5.0, 50.0), (50.0, 50.0)]                             # (mu, shape_inv)
    eta = torch.tensor([[np.float32(math.log(mu))] * n for mu, _ in cells], dtype=torch.float32, device=DEV)
    si = torch.tensor([s for _, s in cells], dtype=torch.float32)
    got = sample_counts(eta, si, seed=SEED, matrix=1, row_index_stride=n).cpu().numpy().astype(np.int64)
    assert (got >= 0).all()
    print()
    for (mu, s), k in zip(cells, got):
        r = float(np.float32(1.0) / np.float32(s))
        z = K.cell_z(k, K.handed_rate(mu), r)                      # "zero": the zero share, 0.89 and 0.86 of the elements at r = 0.02
        print(f"  mu {mu:g} shape_inv {s:g} (r {r:g}): device {fmt_z(z)}")
        assert all(v <= 6.0 for v in z.values()), (mu, s, z)


def test_sampler_is_a_pure_function_of_its_index():
    from velocycle_amd.predictive import sample_counts
    n = 5000
    eta = torch.linspace(-3.0, 6.0, 4 * n, device=DEV).reshape(4, n)
    si = torch.tensor([0.2, 1.0, 2.5, 0.01])
    whole = sample_counts(eta, si, seed=9, draw=3, matrix=1, index_origin=1 << 32, row_index_stride=1 << 32)
    for g in range(4):                     # row by row, cut into two calls at an odd place
        a = sample_counts(eta[g, :1237], si[g:g + 1], seed=9, draw=3, matrix=1, index_origin=(g + 1) << 32)
        b = sample_counts(eta[g, 1237:], si[g:g + 1], seed=9, draw=3, matrix=1, index_origin=((g + 1) << 32) + 1237)
        assert torch.equal(torch.cat([a, b]), whole[g])
    assert not torch.equal(whole, sample_counts(eta, si, seed=9, draw=4, matrix=1, index_origin=1 << 32, row_index_stride=1 << 32))
    assert not torch.equal(whole, sample_counts(eta, si, seed=10, draw=3, matrix=1, index_origin=1 << 32, row_index_stride=1 << 32))


def host_tables(rec):
    """The statistic tables recomputed on the host from the record's own dense replicates."""
    return {m: K.rep_stats(rec.replicates[m].numpy()) for m in rec.replicates}


def assert_tables_follow_replicates(rec, z, tag):
    for m, (gene, cell) in host_tables(rec).items():
        assert np.array_equal(rec.gene_rep[m].numpy(), gene), (tag, m)
        assert np.array_equal(rec.cell_rep[m].numpy(), cell), (tag, m)
        og, oc = K.obs_stats(z["in_" + m])
        assert np.array_equal(rec.gene_obs[m].numpy(), og) and np.array_equal(rec.cell_obs[m].numpy(), oc), (tag, m)


def assert_replicates_within_cap(rec, z, seed, tag, cell_offset=0):
    r64, r32 = K.replicates(z, seed, np.float64, cell_offset), K.replicates(z, seed, np.float32, cell_offset)
    n = sum(v.size for v in r64.values())
    d32 = sum(int((r32[m] != r64[m]).sum()) for m in r64)
    dgpu = sum(int((rec.replicates[m].numpy() != r64[m]).sum()) for m in r64)
    assert all((v >= 0).all() for v in r64.values())
    print(f"{tag}: {n} replicates; float32 restatement differs in {d32}, device in {dgpu}; cap {K.cap(d32, n)}")
    assert dgpu <= K.cap(d32, n), (tag, dgpu, d32)
    return r64


def same_record(a, b):
    ok = all(torch.equal(getattr(a, f)[m], getattr(b, f)[m]) for f in TABLES for m in getattr(a, f))
    if a.replicates is not None and b.replicates is not None:
        ok = ok and all(torch.equal(a.replicates[m], b.replicates[m]) for m in a.replicates)
    return ok


@pytest.mark.parametrize("case", CASES)
def test_fixture_replicates_and_statistics(case):
    from velocycle_amd.predictive import predictive_check
    z = load(case)
    D = int(z["n_draws"])
    eng = engine_of(z)
    rec = predictive_check(eng, draws_of(z), seed=SEED, keep_replicates=D)
    assert rec.n_draws == D and set(rec.replicates) == ({"S", "U"} if str(z["in_kind"]) == "velocity" else {"S"})
    assert_replicates_within_cap(rec, z, SEED, case)
    assert_tables_follow_replicates(rec, z, case)
    eng.close()


@pytest.mark.parametrize("base,Nc,Ng,D", [("vel_mf_joint_nb", 1, 7, 1), ("vel_mf_joint_nb", 63, 1, 3), ("vel_mf_joint_nb", 65, 257, 3),
                                          ("phase_h2_poisson", 65, 257, 1), ("phase_nb", 63, 7, 3), ("vel_mf_dnu2", 1, 1, 1),
                                          ("phase_poisson", 1, 257, 3)])
def test_ragged_shapes(base, Nc, Ng, D):
    from velocycle_amd.predictive import predictive_check
    z = cut(load(base), Ng=Ng, Nc=Nc, D=D)
    eng = engine_of(z)
    rec = predictive_check(eng, draws_of(z), seed=5, keep_replicates=D)
    assert rec.gene_rep["S"].shape == (D, 4, Ng) and rec.cell_rep["S"].shape == (D, Nc) and rec.replicates["S"].shape == (D, Ng, Nc)
    assert_replicates_within_cap(rec, z, 5, f"{base} {Nc} x {Ng} x {D}")
    assert_tables_follow_replicates(rec, z, (base, Nc, Ng, D))
    eng.close()


def test_chunking_storage_and_repetition_give_identical_bits():
    from velocycle_amd.predictive import predictive_check
    from velocycle_amd.tuning import Tuning
    z = cut(load("vel_mf_joint_nb"), Nc=1000)
    dr, D = draws_of(z), int(z["n_draws"])
    e16, e32 = engine_of(z), engine_of(z, tuning=Tuning(count_storage="f32"))
    assert (e16.stats["count_storage"], e32.stats["count_storage"]) == ("u16", "f32")
    a = predictive_check(e16, dr, seed=77, keep_replicates=D)
    assert_tables_follow_replicates(a, z, "1000 cells")
    assert same_record(a, predictive_check(e32, dr, seed=77, keep_replicates=D)), "uint16 and float32 count storage differ"
    assert same_record(a, predictive_check(e16, dr, seed=77, keep_replicates=D)), "two calls differ"
    for cc, cd in ((64, None), (333, None), (None, 1), (None, 5), (100, 3), (1000, D)):
        assert same_record(a, predictive_check(e16, dr, seed=77, keep_replicates=D, chunk_cells=cc, chunk_draws=cd)), (cc, cd)
    part = predictive_check(e16, dr, seed=77, keep_replicates=2)
    assert part.replicates["U"].shape[0] == 2 and torch.equal(part.replicates["U"], a.replicates["U"][:2]) and same_record(
        predictive_check(e16, dr, seed=77), part)
    assert not torch.equal(a.cell_rep["S"], predictive_check(e16, dr, seed=78).cell_rep["S"])
    e16.close(), e32.close()


def raised(z, seed, genes, tops):
    """The fixture with the constant term ν[:, g, 0] of `genes` raised until the gene's largest Poisson rate over cells, draws and
    matrices (after the gamma mixing, for the negative binomial) is tops[i] x 2^20.  Checked with the float64 checker: every rate
    stays inside the sampler's range."""
    lam = K.mixed_rates(z, seed)
    z = dict(z)
    z["draw_ν"] = z["draw_ν"].copy()
    for g, top in zip(genes, tops):
        z["draw_ν"][:, g, 0] += np.float32(math.log(top * K.MU_MAX / max(float(v[:, g].max()) for v in lam.values())))
    after = K.mixed_rates(z, seed)
    assert all(float(v.max()) < 0.97 * K.MU_MAX for v in after.values())
    assert all(abs(max(float(v[:, g].max()) for v in after.values()) / (top * K.MU_MAX) - 1.0) < 1e-5 for g, top in zip(genes, tops))
    return z


@pytest.mark.parametrize("base,Nc,Ng,genes", [("phase_poisson", 130, 9, (2, 6)), ("vel_mf_joint_nb", 65, 7, (2, 5))])
def test_large_counts_through_the_64_bit_statistics(base, Nc, Ng, genes):
    """Two genes of a small cut raised until their largest rates are 0.6 and 0.95 of 2^20, so that counts pass 2^16, a wave's sum of
    k^2 over its 64 cells passes 2^32 (the high half of ppc_wave_sum) and a gene's passes 2^40.  For the Poisson cut the genes' mean
    rates are e^12.5 and e^13.0; no more fits under 2^20, since the count factors put a gene's largest rate 2.3 x above its mean
    (for the negative binomial the gamma, r ~ 3, widens that to ~15 x: mean rates ~e^11)."""
    from velocycle_amd.predictive import predictive_check
    from velocycle_amd.tuning import Tuning
    seed, D = 41, 2
    z = raised(cut(load(base), Nc=Nc, Ng=Ng, D=D), seed, genes, (0.6, 0.95))
    # preconditions, on the float64 checker's replicates: the test cannot stop probing
    r64 = K.replicates(z, seed, np.float64)
    eta64, _ = K.dense_eta(z)
    for m, rep in r64.items():
        assert (rep >= 0).all()
        hot = rep[:, list(genes), :]
        print(f"\n{base} {m}: raised genes' mean rate e^{[round(float(x), 2) for x in eta64[m][:, list(genes)].exp().mean((0, 2)).log()]}, "
              f"largest count {int(hot.max())}, 64-cell sum of k^2 2^{math.log2(float((hot[:, :, :64] ** 2).sum(2).min())):.1f}, "
              f"gene sum of k^2 2^{math.log2(float((hot ** 2).sum(2).max())):.1f}")
    S = r64["S"][:, list(genes), :]
    assert ((S[:, :, :64] ** 2).sum(2) > 2 ** 32).all()                       # both genes, every draw: the first wave of cells
    assert ((S[:, -1] ** 2).sum(1) > 2 ** 40).all() and S.max() > 2 ** 16        # the higher gene's total, every draw
    e16, e32 = engine_of(z), engine_of(z, tuning=Tuning(count_storage="f32"))
    assert (e16.stats["count_storage"], e32.stats["count_storage"]) == ("u16", "f32")
    a = predictive_check(e16, draws_of(z), seed=seed, keep_replicates=D)
    assert_tables_follow_replicates(a, z, base)
    for m in a.replicates:
        got = a.replicates[m].numpy().astype(np.int64)
        assert (got >= 0).all()
        print(f"{base} {m}: {int((got != r64[m]).sum())} of {got.size} replicates differ from the float64 checker's")
        if str(z["in_noisemodel"]) == "Poisson":
            rate = eta64[m][:, list(genes), :].exp().numpy()
            assert (np.abs(got[:, list(genes), :] - rate) <= 8.0 * np.sqrt(rate)).all(), (base, m)
    assert same_record(a, predictive_check(e16, draws_of(z), seed=seed, keep_replicates=D, chunk_cells=64, chunk_draws=1))
    assert same_record(a, predictive_check(e32, draws_of(z), seed=seed, keep_replicates=D)), "uint16 and float32 count storage differ"
    e16.close(), e32.close()


def test_interleaved_batches_report_in_the_caller_s_order():
    from velocycle_amd.predictive import predictive_check
    z0 = load("vel_mf_dnu2")
    Nc, D = z0["in_S"].shape[1], int(z0["n_draws"])
    perm = np.random.default_rng(3).permutation(Nc)
    z = cut(z0, cell_index=perm)
    assert (np.diff(np.argmax(z["in_Db"], 0)) != 0).sum() > 10               # the batches are interleaved: the engine reorders the cells
    e1 = engine_of(z)
    assert e1.stats["onehot_batches"] == 2
    b = predictive_check(e1, draws_of(z), seed=4, keep_replicates=D)
    assert_replicates_within_cap(b, z, 4, "interleaved batches")
    assert_tables_follow_replicates(b, z, "interleaved batches")
    assert same_record(b, predictive_check(e1, draws_of(z), seed=4, keep_replicates=D, chunk_cells=77, chunk_draws=3))
    e1.close()


def test_two_ranks_on_the_halves_of_a_problem():
    from velocycle_amd.engine import HipEngine, shard_bounds
    from velocycle_amd.predictive import merge_check_shards, predictive_check
    z = load("vel_mf_joint_nb")
    spec, dr, D = H.spec_from_fixture(z), draws_of(z), int(z["n_draws"])
    one = HipEngine(spec, device=DEV)
    whole = predictive_check(one, dr, seed=21, keep_replicates=D)
    parts = []
    for r in range(2):
        c0, c1 = shard_bounds(spec.Nc, r, 2)
        e = HipEngine(spec, device=DEV, rank=r, world_size=2)
        parts.append(predictive_check(e, {k: (v[:, c0:c1] if k == "ϕxy" else v) for k, v in dr.items()}, seed=21, keep_replicates=D))
        e.close()
    both = merge_check_shards(parts)
    assert both.n_cells == spec.Nc and same_record(whole, both)
    one.close()


def _fit(noise, n_steps=300):
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    from velocycle_amd.workloads import make_phase_spec
    spec = make_phase_spec(Nc=1500, Ng=100, seed=8, noisemodel=noise)
    eng = HipEngine(spec, device=DEV)
    run = SVIRunner(eng, {"lr": 0.03, "lrd": (0.005 / 0.03) ** (1 / n_steps), "betas": (0.8, 0.99)}, mode="perf", seed=2)
    run.run_perf(n_steps)
    losses = run.perf_losses()
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    return spec, eng


def _as_fixture(spec, draws):
    z = {"in_kind": np.array("phase"), "in_noisemodel": np.array(spec.noisemodel), "in_H": np.array(spec.H), "in_S": spec.S.numpy(),
         "in_count_factor": spec.count_factor.numpy(), "in_with_delta_nu": np.array(False)}
    z.update({"draw_" + k: v.cpu().numpy() for k, v in draws.items()})
    return z


def test_end_to_end_the_poisson_fit_fails_the_variance_check_more_often():
    """NB data of simulate_counts, fitted once with the NB and once with the Poisson phase model (1 500 cells x 100 genes, 300 steps,
    40 draws): the share of genes whose variance has p_mid outside [0.05, 0.95] is strictly larger for the Poisson fit, and every
    p-value equals the float64 checker's on the same draws, except where a differing replicate touches the statistic (then by at most
    its count / D)."""
    from velocycle_amd.predictive import STATISTICS, predictive_check
    D, shares = 40, {}
    for noise in ("NegativeBinomial", "Poisson"):
        spec, eng = _fit(noise)
        names = ["ν", "ϕxy"] + (["shape_inv"] if noise == "NegativeBinomial" else [])
        draws = eng.sample_posterior(names, D, seed=13)
        rec = predictive_check(eng, draws, seed=31, keep_replicates=D)
        z = _as_fixture(spec, draws)
        r64 = assert_replicates_within_cap(rec, z, 31, f"end to end {noise}")["S"]
        assert_tables_follow_replicates(rec, z, noise)
        flips = rec.replicates["S"].numpy() != r64                              # (D, Ng, Nc)
        gene64, cell64 = K.rep_stats(r64)
        T64, Tobs = K.derived(gene64, spec.Nc), K.derived(K.obs_stats(z["in_S"])[0], spec.Nc)
        moved = 0
        for j, s in enumerate(STATISTICS):
            got = rec.gene(s)["S"]
            for name, want in zip(("p_ge", "p_gt", "p_mid"), K.p_values(T64[:, j], Tobs[j])):
                diff = np.abs(got[name].numpy() - want)
                allowed = flips.any(2).sum(0) / D                                # draws of the gene a differing replicate touches
                assert (diff <= allowed + 1e-15).all(), (noise, s, name)
                moved += int((diff > 0).sum())
        lib = rec.library_size()["S"]
        for name, want in zip(("p_ge", "p_gt", "p_mid"), K.p_values(cell64.astype(np.float64), K.obs_stats(z["in_S"])[1])):
            diff = np.abs(lib[name].numpy() - want)
            assert (diff <= flips.any(1).sum(0) / D + 1e-15).all(), (noise, "library", name)
            moved += int((diff > 0).sum())
        pm = rec.gene("variance")["S"]["p_mid"].numpy()
        shares[noise] = float(((pm < 0.05) | (pm > 0.95)).mean())
        print(f"\n[end to end {noise}] genes with the variance's p_mid outside [0.05, 0.95]: {shares[noise]:.3f}; "
              f"{int(flips.sum())} differing replicates moved {moved} p-values")
        eng.close()
    assert shares["Poisson"] > shares["NegativeBinomial"], shares


def _direct_call(eng, n_draws=4):
    one = C.c_void_p(64)                    # never dereferenced: the call is refused before anything is launched
    return eng.lib.vc_predictive_check(eng._h, n_draws, one, 0, one, 0, one, one, one, 0, one, 0, one, 0, 1, 0, 64, 0, n_draws, one, one,
                                       None, None, None, 0, None)


def test_lognormal_and_run_time_sized_engines_are_refused_by_name():
    from velocycle_amd import _lib
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.predictive import predictive_check
    from velocycle_amd.workloads import make_phase_spec
    for kw, word in ((dict(noisemodel="Lognormal"), "Lognormal"), (dict(H=4), "H = 4")):
        eng = HipEngine(make_phase_spec(Nc=200, Ng=20, **kw), device=DEV)
        eng.init_params()
        draws = eng.sample_posterior(["ν", "ϕxy"], 3, seed=1)
        with pytest.raises(NotImplementedError, match=word):
            predictive_check(eng, draws, seed=1)
        assert _direct_call(eng) == _lib.VC_ERR_UNSUPPORTED and word.encode() in eng.lib.vc_last_error(eng._h)
        eng.close()


def test_a_rate_beyond_the_range_latches_the_named_error_and_the_engine_stays_usable():
    from velocycle_amd import _lib
    from velocycle_amd.predictive import SAMPLER_MU_MAX, predictive_check, sample_counts
    with pytest.raises(_lib.CountSamplerRangeError, match="outside the sampler's range"):
        sample_counts(torch.full((100,), math.log(2.0 * SAMPLER_MU_MAX), device=DEV), seed=1)
    ok = sample_counts(torch.full((100,), math.log(0.5 * SAMPLER_MU_MAX), device=DEV), seed=1)
    assert bool((ok > 0.4 * SAMPLER_MU_MAX).all()) and bool((ok < 0.6 * SAMPLER_MU_MAX).all())
    z = load("phase_poisson")
    eng = engine_of(z)
    dr = draws_of(z)
    good = predictive_check(eng, dr, seed=3)
    hot = dict(dr)
    hot["ν"] = dr["ν"].clone()
    hot["ν"][:, 1, 0] = 16.0                                                     # one gene's mean e^16 > 2^20: finite, legal looking
    with pytest.raises(_lib.CountSamplerRangeError, match="outside the count sampler's range"):
        predictive_check(eng, hot, seed=3)
    with pytest.raises(_lib.CountSamplerRangeError):                            # latched: the next call fails too, and so does the status
        predictive_check(eng, dr, seed=3)
    with pytest.raises(_lib.CountSamplerRangeError):
        eng.status()
    eng.clear_status()
    assert eng.status()[0]
    assert same_record(good, predictive_check(eng, dr, seed=3))
    eng.close()
