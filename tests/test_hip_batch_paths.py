"""GPU: one-hot batch offsets on every STEP path, held to the float64 oracle per batch.

d(-ELBO) / d Δν[q, g] of a one-hot batch design is a sum of K_main's partial rows over batch q's chunk range, implemented four times
(vc_common.h: vc_chunk_walk / vc_chunk_walk_lane for 2 <= Nb <= 8 -- the 16 waves of a gene block dealt out to the batches;
vc_dnu_range_issue / _finish and vc_dnu_range_sum for Nb > 8; the fused gene block's own loop over the batches of a Δν wave).  Parity
mode (K_post) is swept by tests/test_hip_sweep.py; here the paths fit() and bench.py run -- the two-launch tail, the three-launch
form, the tutorial flow's merged tail, phases A / B of a sharded rank, the K-particle step -- see Nb in {3, 5, 6, 7, 8} (wave
dealing, 16 not divisible by Nb) and {9, 12, 13} (range sums, several batches per wave), contiguous and interleaved cells, and
planted layouts with an empty batch, a batch of three cells and batches past the 32 rows a range sum requests per trip.

Launch structures per case: the two-launch step (asserted by stats["launches_per_step"]; the joint velocity models with K_main's own
nu_omega partials forced, which the engine declines by itself at Nb >= 12 here), Tuning(tail2=False) -- for the conditioned stage the
merged tail against Tuning(tail_merged=False) -- and whatever the engine selects with nothing forced (checks 1 and 2).

Per case and launch structure:
  1. the FIRST step from the engine's initial parameters (Δν_locs == 0, asserted).  SVIRunner.run_perf(1) on the fused paths runs
     K_main at the initial parameters with the draws of (seed, 0); the tail writes that gradient into the engine's gradient buffer
     (G[po] = gq in the fused gene block, in front of the optimiser update -- unclipped) and samples step 1 without launching its
     likelihood kernel (velocycle_amd/svi.py: _perf_body -> svi_step_fused(n_steps=1); the next K_main is the next call's).  So after
     one step the buffer holds step 0's gradient at the parameters recorded in front of it -- the convention
     tests/test_hip_fused.py::test_fused_step_equals_unfused_sequence relies on for its "last gradient".  Loss to 1e-5, every block to
     assert_step_matches_oracle's bars, every Δν ROW to helpers.assert_dnu_rows_match_oracle (2e-3 of the row's own max-norm: at
     Δν = 0 the prior term vanishes and the row is the likelihood sum over that batch's workgroups);
  2. six steps against the float64 oracle replayed on the same Philox draws (tests/test_hip_fused_oracle.py::_fused_vs_oracle);
  3. six steps against the unfused kernel sequence (adam_impl="hip") at the sweep tolerances of tests/test_hip_fused.py, and the
     launch structures against each other bit for bit."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_hip_fused import _bits_equal, _run, _same
from tests.test_hip_fused_oracle import _fused_vs_oracle
from tests.test_hip_sweep import _problem

pytestmark = pytest.mark.gpu

VCOND_SITES = ["ϕxy", "ν", "Δν", "shape_inv"]
#         kind, guide, noise, H, Hw, Nx, conditioned sites
MODELS = {"phase_h2": ("phase", "meanfield", "NegativeBinomial", 2, 0, 0, []),
          "vjoint_h1": ("velocity", "meanfield", "NegativeBinomial", 1, 1, 2, []),
          "vjoint_h3": ("velocity", "meanfield", "NegativeBinomial", 3, 1, 2, []),       # five Δν waves: up to three batches per wave
          "vjoint_lrmn": ("velocity", "lrmn", "NegativeBinomial", 1, 1, 2, []),
          "vjoint_poisson": ("velocity", "meanfield", "Poisson", 1, 1, 2, []),          # no histogram blocks
          "vcond": ("velocity", "lrmn", "NegativeBinomial", 1, 1, 2, VCOND_SITES)}      # the tutorials' velocity stage (PWL kernel)


def _matrix():
    """(model, layout, Nb, Ng): every Nb in both orders for the phase model and V-joint H = 1; Nb in {3, 7, 12} for the other models;
    the planted layouts for all; one case per model with a second gene block (Ng = 130 at four genes per lane)."""
    out = []
    for m in ("phase_h2", "vjoint_h1"):
        for Nb in (3, 5, 6, 7, 8, 9, 12, 13):
            for layout in ("interleaved", "contiguous"):
                out.append((m, layout, Nb, 130 if (Nb == 6 and layout == "interleaved") else 70))
    for m in ("vjoint_h3", "vjoint_lrmn", "vjoint_poisson", "vcond"):
        out += [(m, "interleaved", 3, 70), (m, "contiguous", 7, 130), (m, "interleaved", 12, 70)]
    for m in MODELS:
        out += [(m, "planted", 9, 70), (m, "planted", 8, 70)]
    return out


def _case(model, layout, Nb, Ng, cells_per_wave=None):
    """(spec, base tuning).  Data of tests.test_hip_sweep._problem; Db overwritten by the layout; for the conditioned stage D is made
    constant within every batch (condition = batch mod 2)."""
    from velocycle_amd.tuning import Tuning
    kind, guide, noise, Hh, Hw, Nx, cond = MODELS[model]
    Nc = 800 if layout == "planted" else 640 + 7 * Nb
    seed = 7000 + 100 * sorted(MODELS).index(model) + 10 * Nb + ("interleaved", "contiguous", "planted").index(layout)
    p = _problem(kind, guide, noise, Hh, Hw, Nb, Nx, cond, Nc=Nc, Ng=Ng, seed=seed)
    ids = H.onehot_layout(Nc, layout, Nb, ids=p.Db.argmax(0))
    p.Db = H.onehot_Db(ids, Nb)
    if cond:
        p.D = torch.stack([((ids % Nx) == x).double() for x in range(Nx)])
    # like with like across the launch structures: the dense histogram tables (what the one-launch tail selects by itself) on both
    # sides; planted: two cells per wave = 8 cells per chunk, batches 0 and 7 then span 50 and 33 chunks
    # ... and, for the joint velocity models, K_main's own nu_omega partials even where the engine declines them (a batch-aligned
    # tiling with more than 12 cells per wave, Nb >= 12 here): the two-launch step on every case, as
    # tests/test_hip_fused.py::test_two_launch_step_medium_sizes forces it; what the engine selects by itself is run beside it
    # Cells per wave: the engine's own tiling for the interleaved layouts (~22 chunks per gene block at these sizes); two for the
    # contiguous ones as well (~85 chunks).  With ~3 chunks per batch the LAST wave of a batch's wave group (Nb = 6: six waves for
    # the last batch, Nb = 7: four) has no chunk at all, and a sum that leaves that wave out is still right: measured -- a build
    # with exactly that mistake passed every Nb = 6, 7 case on the engine's own tiling.
    hist = noise == "NegativeBinomial" and "shape_inv" not in cond
    tun = Tuning(hist_dense="dense" if hist else None, genes_per_lane=4 if Ng > 70 else 0, cells_per_wave=cells_per_wave if
                 cells_per_wave is not None else (0 if layout == "interleaved" else 2),
                 pw_inline="force" if (kind == "velocity" and not cond) else None)
    return H.spec_from_problem(p), tun


OPT = {"lr": 0.03, "lrd": 0.995, "betas": (0.8, 0.99)}


def _first_step(spec, tuning, seed, label):
    """Check 1 of the module docstring; returns (engine stats, worst err / bar of the Δν rows or None)."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    e = HipEngine(spec, tuning=tuning)
    r = SVIRunner(e, OPT, mode="perf", seed=seed)
    assert r.adam_impl == "fused3" and not r.use_graph
    flat0 = e.params.detach().clone()
    par0 = {k: v.detach().cpu().clone() for k, v in e.named().items()}
    learned = "Δν" not in spec.condition_on
    if learned:
        assert not bool(par0["Δν_locs"].any())          # the prior term of its gradient is exactly zero
    r.run_perf(1)
    loss = r.perf_losses()[0]
    grads = {k: v.detach().cpu().clone() for k, v in e.named(e.grad).items()}
    stats = dict(e.stats)
    assert e.status() == (True, -1, 0) and stats["onehot_batches"] == spec.Nb and not stats["generic"], stats
    e.close()
    eps = H.philox_eps_list(spec, flat0, seed, 1)[0]
    _, g64 = H.assert_grads_match_oracle(loss, grads, par0, spec, eps)
    ratio = None
    if learned:
        ratio = float(H.assert_dnu_rows_match_oracle(grads["Δν_locs"], g64["Δν_locs"], label).max())
    return stats, ratio


@pytest.mark.parametrize("model,layout,Nb,Ng", _matrix())
def test_fused_step_paths_hold_every_batch_row(model, layout, Nb, Ng):
    spec, base = _case(model, layout, Nb, Ng)
    seed, n = 3, 6
    vcond = model == "vcond"
    other = base.replace(tail_merged=False) if vcond else base.replace(tail2=False)
    runs, worst = {}, {}
    for name, tun in (("two", base), ("other", other)):
        label = f"{model} {layout} Nb={Nb} Ng={Ng} [{name}]"
        stats, worst[name] = _first_step(spec, tun, seed, label)
        if name == "two":
            # the launch structure fit() and bench.py run: two launches -- the one-launch tail, or the merged tail of the tutorial
            # flow, whose likelihood kernel keeps the nu_omega partials per lane (one condition per batch-aligned workgroup)
            assert stats["launches_per_step"] == 2, stats
            if vcond:
                assert stats["pw_lane"], stats
        elif not vcond:
            assert stats["launches_per_step"] == 3, stats
        _fused_vs_oracle(spec, n=n, seed=seed, tuning=tun)
        runs[name] = _run(spec, "fused3", n, False, seed=seed, tuning=tun)
    ref = _run(spec, "hip", n, False, seed=seed, tuning=base)
    got = runs["two"]
    assert got["status"][0] and np.allclose(got["l"], ref["l"], rtol=2e-6, atol=0), (got["l"], ref["l"])
    _same(got["p"], ref["p"], "params after six steps, fused vs unfused", rtol=2e-4, atol=2e-5)
    _same(got["m"], ref["m"], "exp_avg after six steps, fused vs unfused", rtol=2e-3, atol=5e-3)
    _bits_equal(runs["two"], runs["other"], f"{model} {layout} Nb={Nb}: launch structures")
    # ... and what the engine selects with nothing forced (its default; three launches with the cell blocks' own nu_omega partials
    # where it declines K_main's, the histogram lists there)
    plain = base.replace(pw_inline=None, hist_dense=None)
    if plain != base:
        stats, worst["plain"] = _first_step(spec, plain, seed, f"{model} {layout} Nb={Nb} Ng={Ng} [nothing forced]")
        assert stats["launches_per_step"] in (2, 3), stats
        _fused_vs_oracle(spec, n=n, seed=seed, tuning=plain)
        worst[f"nothing forced ({stats['launches_per_step']} launches)"] = worst.pop("plain")
    if worst["two"] is not None:
        print(f"[dnu rows, fused step] {model} {layout} Nb={Nb} Ng={Ng}: worst err / bar "
              + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("model", ["phase_h2", "vjoint_h1"])
def test_parity_mode_on_the_planted_layout(model):
    """K_post (vc_dnu_range_sum for every batch) on the planted Nb = 9 layout at 8 cells per chunk: ranges past the 32 rows of one trip,
    which the sweep's own layouts (at most ~25 chunks per batch) do not reach.  `_check` of tests/test_hip_sweep.py, Δν rows included."""
    from tests.test_hip_sweep import _check
    from velocycle_amd.tuning import Tuning
    kind, guide, noise, Hh, Hw, Nx, cond = MODELS[model]
    p = _problem(kind, guide, noise, Hh, Hw, 9, Nx, cond, Nc=800, Ng=70, seed=8100 + Hh)
    p.Db = H.onehot_Db(H.onehot_layout(800, "planted", 9), 9)
    k = _check(p, None, Tuning(cells_per_wave=2))
    assert k.startswith(f"vc_main_kernel<{Hh},0,"), k


# ---- sharded: phases A / B of three ranks on one device (tests/test_hip_sharded_step.py) ------------------------------------------

def _sharded_state(ranks):
    par = {k: v.detach().cpu().clone() for k, v in ranks[0].e.named().items()}
    par["ϕxy_locs"] = torch.cat([r.e.view(r.e.params, "ϕxy_locs").detach().cpu() for r in ranks])
    return par


@pytest.mark.parametrize("model", ["vjoint_h1", "phase_h2"])
@pytest.mark.parametrize("layout,Nb", [("contiguous", 5), ("interleaved", 7), ("planted", 9)])
def test_sharded_step_holds_every_batch_row(model, layout, Nb):
    """world = 3: with contiguous batches ranks lack whole batches (empty chunk ranges, their partial is the prior term alone); the
    planted layout leaves rank 0 with one batch.  The summed gradient of the first step (left in `grad` by phase B; phi_xy blocks
    concatenated over the ranks) against the oracle as above, six steps against the oracle replay like
    test_sharded_sequence_matches_oracle_on_a_slice_of_the_benchmark_data, replicated state bit-identical on the ranks."""
    from velocycle_amd.engine import HipEngine
    from tests.test_hip_sharded_step import _Rank, _run_sharded, OPT as SOPT
    # (one cell per wave = 4 cells per chunk: every wave of a batch's wave group has chunks on every rank that holds the batch, and
    # the planted batches 0 and 7 keep more than 32 chunks on the rank that holds them)
    spec, tun = _case(model, layout, Nb, 70, cells_per_wave=1)
    world, n, seed = 3, 6, 5
    nz = lambda t: torch.nan_to_num(t, neginf=-1e30)
    probe = [_Rank(spec, r, world, seed, tun) for r in range(world)]
    par0 = _sharded_state(probe)
    for r in probe:
        r.e.close()
    assert not bool(par0["Δν_locs"].any())
    e0 = HipEngine(spec)
    e0.set_params(par0)
    flat0 = e0.params.detach().clone()
    e0.close()
    eps = H.philox_eps_list(spec, flat0, seed, n)
    # first step
    ranks = _run_sharded(spec, world, 1, seed, tun)
    grads = {k: v.detach().cpu().clone() for k, v in ranks[0].e.named(ranks[0].e.grad).items()}
    grads["ϕxy_locs"] = torch.cat([r.e.view(r.e.grad, "ϕxy_locs").detach().cpu() for r in ranks])
    loss = float(ranks[0].ring[0].item())
    for r in ranks:
        assert r.e.status() == (True, -1, 0) and r.e.stats["onehot_batches"] == Nb
        r.e.close()
    _, g64 = H.assert_grads_match_oracle(loss, grads, par0, spec, eps[0])
    ratio = H.assert_dnu_rows_match_oracle(grads["Δν_locs"], g64["Δν_locs"], f"sharded {model} {layout} Nb={Nb}")
    print(f"[dnu rows, sharded step] {model} {layout} Nb={Nb}: worst err / bar {ratio.max():.2e}")
    # six steps
    ranks = _run_sharded(spec, world, n, seed, tun)
    ng = ranks[0].e.header + ranks[0].e.n_global
    for r in ranks[1:]:
        assert torch.equal(nz(r.e.params[:ng]), nz(ranks[0].e.params[:ng]))
        assert torch.equal(r.m[: ng - 4], ranks[0].m[: ng - 4]) and torch.equal(r.v[: ng - 4], ranks[0].v[: ng - 4])
        assert torch.equal(r.ring[:n], ranks[0].ring[:n]) and int(r.sd.item()) == n
    losses = ranks[0].ring[:n].cpu().numpy()
    got = {k: v.numpy().astype(np.float64) for k, v in _sharded_state(ranks).items()}
    for r in ranks:
        assert r.e.status() == (True, -1, 0)
        r.e.close()
    opt = {"lr": SOPT["lr"], "lrd": SOPT["lrd"], "betas": (SOPT["b1"], SOPT["b2"])}
    l64, par64 = H.oracle_replay(spec, opt, par0, eps, torch.float64)
    l32, par32 = H.oracle_replay(spec, opt, par0, eps, torch.float32)
    l64, l32 = np.array(l64), np.array(l32)
    rel_hip, rel_32 = np.abs(losses - l64) / np.abs(l64), np.abs(l32 - l64) / np.abs(l64)
    assert rel_hip[:5].max() <= 1e-5, rel_hip[:5]
    assert (rel_hip <= np.maximum(1e-5, 4 * np.maximum.accumulate(rel_32))).all(), (rel_hip.max(), rel_32.max())
    H.assert_params_track_oracle(got, {k: v.numpy() for k, v in par64.items()}, {k: v.double().numpy() for k, v in par32.items()})


# ---- K particles: vc_svi_run_particles (K_pre / K_post of all particles, K_fin + average + optimiser) -----------------------------

@pytest.mark.parametrize("layout,Nb", [("interleaved", 7), ("planted", 9)])
def test_particle_step_with_many_batches(layout, Nb):
    """SVIRunner(num_particles=3), eight steps: the kernels compiled for the configuration's signature against the run-time-flag
    kernels (Tuning(no_tail_spec=True)) like tests/test_hip_tail_spec.py::test_particle_step_specialisation_is_bit_identical, and the C
    call against the host loop of K x vc_elbo_grad (Tuning(particles_host_loop=True)) like tests/test_hip_particles.py: parameters,
    moments and losses bit for bit."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    spec, tun = _case("vjoint_h1", layout, Nb, 70)
    out = []
    for t in (tun, tun.replace(no_tail_spec=True), tun.replace(particles_host_loop=True)):
        e = HipEngine(spec, tuning=t)
        if t.no_tail_spec:
            assert e.stats["tail_spec_name"] == "generic"
        assert e.stats["onehot_batches"] == Nb
        r = SVIRunner(e, OPT, mode="perf", seed=9, num_particles=3)
        assert r.adam_impl == "hip"
        r.run_perf(8)
        out.append((e.params.clone().cpu(), r.opt.m.clone().cpu(), r.opt.v.clone().cpu(), np.array(r.perf_losses()), e.status()))
        e.close()
    nz = lambda t: torch.nan_to_num(t, neginf=-1e30)
    a = out[0]
    assert a[4] == (True, -1, 0) and len(a[3]) == 8 and np.isfinite(a[3]).all()
    for b in out[1:]:
        assert torch.equal(nz(a[0]), nz(b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert b[4] == (True, -1, 0)
