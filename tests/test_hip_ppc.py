"""GPU: the device count sampler (vc_sample_counts) and the posterior predictive check (vc_predictive_check) against the float64
checker (tests/ppc_checker.py).  Counts are compared for EQUALITY; a float32 evaluation may land on the other side of an accept /
floor / search decision, so a share of elements may differ: at most SAFETY (4) x the number the float32 restatement itself differs
from the float64 one in on the same inputs, at least 16 elements.  Statistics are compared exactly."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import ppc_checker as K
from tests.test_hip_pointwise import cut, draws_of, engine_of
from tests.test_pointwise_cpu import CASES, load
from tests.test_ppc_cpu import SEED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_CELL = 1 << 18                      # samples per grid cell: 16 cells = 2^22 elements
TABLES = ("gene_rep", "cell_rep", "gene_obs", "cell_obs")


def device_grid(n, seed, draw):
    """vc_sample_counts over ppc_checker.GRID in the layout of ppc_checker.sample_grid."""
    from velocycle_amd.predictive import sample_counts
    eta, r = K.grid_inputs(n)
    n_p = sum(1 for _, rr in K.GRID if rr is None)
    assert all(rr is None for _, rr in K.GRID[:n_p]) and all(rr is not None for _, rr in K.GRID[n_p:])
    e = torch.tensor(eta, device=DEV)
    kp = sample_counts(e[:n_p * n], seed=seed, draw=draw, matrix=0, index_origin=0)
    si = torch.tensor([1.0 / np.float32(rr) for _, rr in K.GRID[n_p:]], dtype=torch.float32)
    kn = sample_counts(e[n_p * n:].reshape(-1, n), si, seed=seed, draw=draw, matrix=1, index_origin=n_p * n, row_index_stride=n)
    return torch.cat([kp, kn.reshape(-1)]).cpu().numpy().astype(np.int64), si.numpy()


def test_sampler_against_the_float64_checker_and_the_exact_moments():
    got, si = device_grid(N_CELL, SEED, 0)
    assert got.size >= 1 << 22 and (got >= 0).all()
    # the checker divides by the same float32 r = 1 / shape_inv the device forms
    n_p = len(K.GRID) - si.size
    r32 = [None] * n_p + [np.float32(1.0) / s for s in si]
    eta, _ = K.grid_inputs(N_CELL)
    idx = np.arange(eta.size, dtype=np.uint64)
    k64, k32 = np.empty_like(got), np.empty_like(got)
    for i, rr in enumerate(r32):
        sl = slice(i * N_CELL, (i + 1) * N_CELL)
        rv = None if rr is None else np.full(N_CELL, rr, dtype=np.float32)
        k64[sl] = K.sample_counts(eta[sl], rv, SEED, 0, 0 if rr is None else 1, idx[sl], np.float64)
        k32[sl] = K.sample_counts(eta[sl], rv, SEED, 0, 0 if rr is None else 1, idx[sl], np.float32)
    d32, dgpu = int((k32 != k64).sum()), int((got != k64).sum())
    print(f"\n[sampler, {got.size} elements] float32 restatement differs from float64 in {d32} (share {d32 / got.size:.2e}), "
          f"device in {dgpu} (share {dgpu / got.size:.2e}); cap {K.cap(d32, got.size)}")
    for i, (mu, r) in enumerate(K.GRID):
        sl = slice(i * N_CELL, (i + 1) * N_CELL)
        z = K.moment_z(got[sl], K.exact_moments(mu, r))
        print(f"  mu {mu} r {r}: device |z| mean {z['mean']:.2f} variance {z['var']:.2f} zero share {z['zero']:.2f}; "
              f"differing float32 {int((k32[sl] != k64[sl]).sum())} device {int((got[sl] != k64[sl]).sum())}")
        assert all(v <= 6.0 for v in z.values()), (mu, r, z)
    assert 0 < d32 < 1e-3 * got.size
    assert dgpu <= K.cap(d32, got.size), (dgpu, d32)


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
