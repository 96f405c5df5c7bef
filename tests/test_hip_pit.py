"""GPU: the predictive PIT (velocycle_amd.predictive.predictive_pit / vc_predictive_pit, csrc/vc_pit.hip) against the float64 checker
(tests/pit_checker.py) on the pointwise fixtures (tests/golden/ref_pointwise_*.npz).  Bar: 4 x the worst error ratio the checker's
own float32 evaluation shows over the fixtures (tests/test_pit_cpu.bars), in accuracy units s = eps32 (1 + A) F_hi + eps32; no element
is left out of any comparison.  The histograms are integers: every statement about them is exact."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pit_checker as Q
from tests.test_hip_pointwise import cut, draws_of, engine_of
from tests.test_pit_cpu import SEED, bars, checked
from tests.test_pointwise_cpu import CASES, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = np.float32
BELOW_ONE = F32(0.99999994)


def assert_record(tag, rec, e64, bins):
    """Everything one record must satisfy against the float64 evaluation e64 of the same problem, seed and cell offset."""
    bar = bars()
    got = {}
    for i, m in enumerate(e64):
        lo, hi, u = (rec.pointwise[m][j].numpy() for j in range(3))
        Ng, Nc = lo.shape
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(u).all(), (tag, m)
        assert (lo >= 0).all() and (lo <= hi).all() and (hi <= 1).all() and (u >= 0).all() and (u < 1).all(), (tag, m)
        # u: the float32 fma of the device's own F's with the checker's v, within one ulp
        v = e64[m]["v"].numpy()
        want = np.clip((v * (hi - lo).astype(np.float64) + lo.astype(np.float64)).astype(F32), F32(0), BELOW_ONE)
        assert (np.abs(u - want) <= np.spacing(want)).all(), (tag, m, float(np.abs(u - want).max()))
        got[m] = {"F_lo": lo, "F_hi": hi, "u": u}
        # the tables are the histograms of the device's own u, exactly; every row is complete
        gene, cell = Q.histograms(u, bins, F32)
        assert np.array_equal(rec.gene_hist[m].numpy(), gene) and np.array_equal(rec.cell_hist[m].numpy(), cell), (tag, m)
        assert (rec.gene_hist[m].sum(1) == Nc).all() and (rec.cell_hist[m].sum(1) == Ng).all(), (tag, m)
        # against the float64 histograms: a gene may differ only by its elements whose float64 u lies within its own bar of a bin edge
        u64, s = e64[m]["u"].numpy(), e64[m]["s"].numpy()
        gene64, _ = Q.histograms(u64, bins)
        near = Q.near_edge(u64, bar * s, bins)
        l1 = np.abs(gene - gene64).sum(1)
        assert (l1 <= 2 * near.sum(1)).all(), (tag, m, l1.max(), int(near.sum()))
        print(f"{tag} {m}: {int(near.sum())} of {near.size} elements within their bar of a bin edge, histogram L1 difference {int(l1.sum())}")
    r = Q.ratios(got, e64)
    print(f"{tag}: error ratios (accuracy units) " + ", ".join(f"{q} {r[q]:.3f}" for q in Q.QUANT) + f" (bar {bar:.3f})")
    for q in Q.QUANT:
        assert r[q] <= bar, (tag, q, r[q], bar)
    return r


def same_bits(a, b):
    for f in ("gene_hist", "cell_hist", "pointwise"):
        for m in getattr(a, f):
            if not torch.equal(getattr(a, f)[m], getattr(b, f)[m]):
                return False
    return (a.n_draws, a.bins, a.seed) == (b.n_draws, b.bins, b.seed)


@pytest.mark.parametrize("case", CASES)
def test_fixture_within_the_measured_bar(case):
    from velocycle_amd.predictive import predictive_pit
    z, e64 = checked(case)
    eng = engine_of(z)
    rec = predictive_pit(eng, draws_of(z), seed=SEED, return_pointwise=True)
    assert rec.n_draws == int(z["n_draws"]) and rec.bins == 20 and set(rec.gene_hist) == set(e64)
    assert_record(case, rec, e64, 20)
    without = predictive_pit(eng, draws_of(z), seed=SEED)
    assert without.pointwise is None and all(torch.equal(without.gene_hist[m], rec.gene_hist[m]) for m in e64)
    eng.close()


@pytest.mark.parametrize("base,Nc,Ng,D,bins", [("vel_mf_joint_nb", 1, 7, 1, 20), ("vel_mf_joint_nb", 63, 1, 3, 2),
                                               ("vel_mf_joint_nb", 65, 257, 2, 64), ("vel_mf_joint_nb", 1000, 7, 50, 20),
                                               ("phase_h2_poisson", 65, 257, 3, 2), ("vel_mf_dnu2", 63, 7, 50, 64)])
def test_ragged_shapes_against_the_checker(base, Nc, Ng, D, bins):
    from velocycle_amd.predictive import predictive_pit
    z = cut(load(base), Ng=Ng, Nc=Nc, D=D)
    eng = engine_of(z)
    rec = predictive_pit(eng, draws_of(z), seed=5, bins=bins, return_pointwise=True)
    assert rec.gene_hist["S"].shape == (Ng, bins) and rec.cell_hist["S"].shape == (Nc, bins) and rec.pointwise["S"].shape == (3, Ng, Nc)
    assert_record(f"{base} {Nc} x {Ng} x {D}, {bins} bins", rec, Q.evaluate(z, 5), bins)
    eng.close()


@pytest.mark.parametrize("base", ["phase_nb", "phase_poisson"])
def test_deep_tails_stay_finite_ordered_and_within_the_bar(base):
    """Zeros where the mean is largest (F_hi = pmf(0) ~ 0) and 60 000 in cells of a low-expressed gene (F_lo ~ 1 after 60 000 terms
    that grow by hundreds of orders of magnitude on the way down to the mode)."""
    from velocycle_amd.predictive import predictive_pit
    z = cut(load(base), Ng=7, Nc=65, D=2)
    mu = Q.etas(Q.PC.problem_of(z))["S"].exp().mean(0).numpy()              # (Ng, Nc)
    S = z["in_S"].copy()
    top = np.argsort(mu.ravel())[-8:]
    S.ravel()[top] = 0.0
    low = int(np.argmin(mu.mean(1)))
    S[low, [0, 31, 64]] = 60000.0
    z["in_S"] = S
    e64 = Q.evaluate(z, 9)
    first, second = e64["S"]["F_hi"].numpy().ravel()[top], e64["S"]["F_lo"].numpy()[low, [0, 31, 64]]
    print(f"{base}: float64 F_hi of the zeros {first.max():.2e} (means {mu.ravel()[top].min():.0f} ..), F_lo of the 60 000s {second.min():.12f} "
          f"(mean {mu[low].mean():.3g})")
    assert first.max() < 1e-2 and second.min() > 1 - 1e-6                  # (the negative binomial's pmf(0) at r ~ 1: 2e-3)
    eng = engine_of(z)
    assert eng.stats["count_storage"] == "u16"
    rec = predictive_pit(eng, draws_of(z), seed=9, return_pointwise=True)
    assert_record(f"deep tails {base}", rec, e64, 20)
    lo, hi = rec.pointwise["S"][0].numpy(), rec.pointwise["S"][1].numpy()
    print(f"{base}: device F_hi of the zeros {hi.ravel()[top].max():.2e}, F_lo of the 60 000s {lo[low, [0, 31, 64]]}")
    # the unit at A ~ 1.5e6 would let a gross tail error through: the device's own values, directly
    assert hi.ravel()[top].max() < 1e-2 and lo[low, [0, 31, 64]].min() > 0.9, (base, hi.ravel()[top].max(), lo[low, [0, 31, 64]])
    eng.close()


def test_storage_repeat_and_chunking_give_identical_bits():
    from velocycle_amd.predictive import predictive_pit
    from velocycle_amd.tuning import Tuning
    z = cut(load("vel_mf_joint_nb"), Nc=1000, Ng=40, D=4)
    dr = draws_of(z)
    e16, e32 = engine_of(z), engine_of(z, tuning=Tuning(count_storage="f32"))
    assert (e16.stats["count_storage"], e32.stats["count_storage"]) == ("u16", "f32")
    a = predictive_pit(e16, dr, seed=77, return_pointwise=True)
    assert same_bits(a, predictive_pit(e32, dr, seed=77, return_pointwise=True)), "uint16 and float32 count storage differ"
    assert same_bits(a, predictive_pit(e16, dr, seed=77, return_pointwise=True)), "two calls differ"
    for chunk in (64, 1000, None, 77):
        assert same_bits(a, predictive_pit(e16, dr, seed=77, return_pointwise=True, chunk_cells=chunk)), f"chunk_cells={chunk} differs"
    other = predictive_pit(e16, dr, seed=78, return_pointwise=True)
    assert torch.equal(other.pointwise["U"][:2], a.pointwise["U"][:2]) and not torch.equal(other.pointwise["U"][2], a.pointwise["U"][2])
    e16.close(), e32.close()


def test_interleaved_batches_report_in_the_caller_s_order():
    from velocycle_amd.predictive import predictive_pit
    z0 = load("vel_mf_dnu2")
    Nc = z0["in_S"].shape[1]
    perm = np.random.default_rng(3).permutation(Nc)
    z = cut(z0, cell_index=perm)
    assert (np.diff(np.argmax(z["in_Db"], 0)) != 0).sum() > 10               # the batches are interleaved: the engine reorders the cells
    e0, e1 = engine_of(z0), engine_of(z)
    assert e1.stats["onehot_batches"] == 2
    a = predictive_pit(e0, draws_of(z0), seed=SEED, return_pointwise=True)
    b = predictive_pit(e1, draws_of(z), seed=SEED, return_pointwise=True)
    assert_record("interleaved batches", b, Q.evaluate(z, SEED), 20)
    # the CDFs travel with their cell, bit for bit; v belongs to the position (the global cell index), so u is the fma of both
    for m in ("S", "U"):
        assert torch.equal(a.pointwise[m][:2][:, :, perm], b.pointwise[m][:2]), m
    assert same_bits(b, predictive_pit(e1, draws_of(z), seed=SEED, return_pointwise=True, chunk_cells=77))
    e0.close(), e1.close()


def test_two_ranks_on_the_halves_of_a_problem():
    from velocycle_amd.engine import HipEngine, shard_bounds
    from velocycle_amd.predictive import merge_pit_shards, predictive_pit
    z = load("vel_mf_joint_nb")
    spec, dr = H.spec_from_fixture(z), draws_of(z)
    one = HipEngine(spec, device=DEV)
    whole = predictive_pit(one, dr, seed=21, return_pointwise=True)
    parts = []
    for r in range(2):
        c0, c1 = shard_bounds(spec.Nc, r, 2)
        e = HipEngine(spec, device=DEV, rank=r, world_size=2)
        parts.append(predictive_pit(e, {k: (v[:, c0:c1] if k == "ϕxy" else v) for k, v in dr.items()}, seed=21, return_pointwise=True))
        e.close()
    assert same_bits(whole, merge_pit_shards(parts))                          # the second rank took v at ITS global cell indices
    half = spec.Nc // 2
    assert not torch.equal(parts[0].pointwise["S"][2][:, :half], parts[1].pointwise["S"][2][:, :half])
    one.close()


@pytest.mark.parametrize("case", ["vel_mf_joint_nb", "phase_poisson"])
def test_calibration_of_the_sampler_s_counts_end_to_end(case):
    """Two pieces that share no code: counts drawn by the device's exact sampler (predictive_check) under one draw, scored by the
    PIT kernel under that draw, are uniform (pooled and per gene); scored with shape_inv / 8 they are far from it."""
    from velocycle_amd.predictive import predictive_check, predictive_pit
    z = cut(load(case), D=1)
    dr = draws_of(z)
    eng = engine_of(z)
    rep = predictive_check(eng, dr, seed=33, keep_replicates=1).replicates
    eng.close()
    z2 = dict(z)
    for m, k in rep.items():
        z2["in_" + m] = k[0].numpy().astype(np.float32)
    eng = engine_of(z2)
    rec = predictive_pit(eng, dr, seed=34)
    for m, p in rec.pooled().items():
        zg = rec.gene()[m]["z"]
        print(f"{case} {m}: pooled z {p['z']:.2f}, worst gene z {float(zg.max()):.2f}, edge share {p['edge_share']:.3f}")
        assert p["z"] < Q.GOF_Z and float(zg.max()) < Q.GOF_Z, (case, m, p["z"], float(zg.max()))
    if "shape_inv" in dr:
        wrong = dict(dr)
        wrong["shape_inv"] = dr["shape_inv"] / 8
        for m, p in predictive_pit(eng, wrong, seed=34).pooled().items():
            print(f"{case} {m} scored with shape_inv / 8: pooled z {p['z']:.1f}, edge share {p['edge_share']:.3f}")
            assert p["z"] > 60 and p["edge_share"] > 0.15, (case, m, p)
    eng.close()


def _direct_call(eng, gene, cell, n_draws=3):
    one = C.c_void_p(64)                    # never dereferenced: the call is refused before anything is launched
    vp = lambda t: C.c_void_p(t.data_ptr())
    return eng.lib.vc_predictive_pit(eng._h, n_draws, one, 0, one, 0, one, one, one, 0, one, 0, one, 0, 1, 20, 0, 64, vp(gene), vp(cell), None,
                                     None)


def test_unsupported_engines_are_refused_by_name():
    from velocycle_amd import _lib
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.predictive import predictive_pit
    from velocycle_amd.workloads import make_phase_spec
    half, huge = make_phase_spec(Nc=200, Ng=20), make_phase_spec(Nc=200, Ng=20)
    half.S, huge.S = half.S.clone(), huge.S.clone()
    half.S[3, 5] += 0.5
    huge.S[3, 5] = 16777216.0                                               # 2^24: float32 cannot count down from here
    for spec, word in ((make_phase_spec(Nc=200, Ng=20, noisemodel="Lognormal"), "Lognormal"), (make_phase_spec(Nc=200, Ng=20, H=4), "H = 4"),
                       (half, "non-integer counts"), (huge, "outside [0, 2^24)")):
        eng = HipEngine(spec, device=DEV)
        eng.init_params()
        names = ["ν", "ϕxy"] + (["shape_inv"] if spec.noisemodel == "NegativeBinomial" else [])
        draws = eng.sample_posterior(names, 3, seed=1)
        with pytest.raises(NotImplementedError, match=re.escape(word)):
            predictive_pit(eng, draws, seed=1)
        with pytest.raises(NotImplementedError, match=re.escape(word)):      # (the engine's answer is cached: the second call agrees)
            predictive_pit(eng, draws, seed=1, chunk_cells=64)
        gene = torch.zeros((1, 20, 20), dtype=torch.int64, device=DEV)
        cell = torch.zeros((1, 200, 20), dtype=torch.int64, device=DEV)
        assert _direct_call(eng, gene, cell) == _lib.VC_ERR_UNSUPPORTED and word.encode() in eng.lib.vc_last_error(eng._h)
        torch.cuda.synchronize()
        assert int(gene.sum()) == 0 and int(cell.sum()) == 0                # nothing was launched
        eng.close()
