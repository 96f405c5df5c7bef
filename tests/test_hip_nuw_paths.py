"""GPU: the angular-speed coefficients on every step path, every gradient row held to the float64 oracle PER CONDITION.

d loglik / d nu_omega[x, h] = sum_c A3_c D[x, c] zeta_omega_h(phi_c), one row per condition x, is written many times: the U-only
likelihood kernel's per-lane accumulators, stored in the columns of the workgroup's condition (PWL: `my_cond` from the tile table's
batch | condition << 16); K_main's wave reduction over the W rows (vc_put_w) in the U-only and the S+U kernel; the cell blocks' own
partials PW (vc_post_cell_block's 1024-cell blocks with conditions 0 / 1 through dx01[] and the others through Dm, the tails' 256-cell
blocks, phase A's exchange slots, the run-time-sized set); and behind all of them the column sums (vc_nuw_sums_issue / _finish with
rows in registers up to 768 partial rows and vc_col_sum_d beyond, coefficients dealt out as wv + nwv q and a third loop for the rest;
vc_nuw_sums_direct and its folded peer-to-peer branch; the merged tail's float4 copy; K_fin).  A block-wide bar cannot see one
condition (tests/test_nuw_rows_cpu.py: a three-cell condition's whole row can lie under it), so here every row is held to
helpers.assert_nuw_rows_match_oracle -- 2e-3 of the row's own likelihood part -- and the angular speed of every cell to
helpers.assert_omega_matches_oracle, on the cases of tests/test_nuw_rows_cpu.py: a condition of three cells, conditions without any
cell, conditions that cut through the batches, nu_omega 0.2 apart between conditions.  Every path is asserted through engine.stats.

Fused paths, per case and launch structure: the FIRST step from the initial parameters with the Philox draws (loss, every block at
assert_grads_match_oracle's bars, the rows, omega of the K_pre sample at step 0 and of the chain's sample of step 1), six steps against
the float64 oracle replay, and the launch structures against each other bit for bit.  Unfused paths (elbo_grad with host draws):
the perturbed point of tests/test_nuw_rows_cpu.py::point."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_hip_fused import _bits_equal, _run
from tests.test_hip_fused_oracle import _fused_vs_oracle
from tests.test_nuw_rows_cpu import CASES, MODELS, PWL_SHAPES, Case, build, point

pytestmark = pytest.mark.gpu

OPT = {"lr": 0.03, "lrd": 0.995, "betas": (0.8, 0.99)}
SEED, NSTEPS = 3, 6
WORST = {}          # path -> worst err / bar over the run so far: rows of conditions with cells, rows of conditions without, omega


def _note(path, rows, omega, spec):
    """Prints the running worst of a path (copied into DESIGN section 4)."""
    cells = (spec.D.sum(1) > 0).numpy()
    w = WORST.setdefault(path, [0.0, 0.0, 0.0])
    w[0] = max(w[0], max(float(v[cells].max()) for v in rows.values()))
    w[1] = max(w[1], max(float(v[~cells].max(initial=0.0)) for v in rows.values()))
    w[2] = max(w[2], omega)
    print(f"[nuw rows] {path}: worst row err / bar so far {w[0]:.2e} (conditions with cells), {w[1]:.2e} (without); "
          f"worst omega err / bar {w[2]:.2e}")


def _select(models, layouts, shapes, Nc=800, Ng=70, orders=("contiguous", "interleaved")):
    return [c for c in CASES if c.model in models and c.layout in layouts and (c.Nx, c.Hw) in shapes and c.Nc == Nc and c.Ng == Ng
            and c.order in orders]


def _tuning(case, **kw):
    """Like with like across launch structures: the dense histogram tables wherever shape_inv is learned (what the one-launch tail
    selects by itself); two cells per wave: ~100 batch-aligned workgroups per gene block, the three-cell batch in one of its own."""
    from velocycle_amd.tuning import Tuning
    learned_si = "shape_inv" not in MODELS[case.model][6]
    kw.setdefault("cells_per_wave", 2)
    return Tuning(hist_dense="dense" if learned_si else None, genes_per_lane=4 if case.Ng > 70 else 0, **kw)


def _spec(case):
    return H.spec_from_problem(build(case)[0])


def _first_step(spec, tuning, label):
    """The first fused step; returns (engine stats, row ratios, worst omega ratio)."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    e = HipEngine(spec, tuning=tuning)
    r = SVIRunner(e, OPT, mode="perf", seed=SEED)
    assert r.adam_impl == "fused3" and not r.use_graph
    flat0 = e.params.detach().clone()
    par0 = {k: v.detach().cpu().clone() for k, v in e.named().items()}
    # the sample of step 0 by the unfused sampler (K_pre) ...
    e.sample_guide(eps=None, seed=SEED, step=0)
    omega0 = e.read_site("ω")
    r.run_perf(1)
    loss = r.perf_losses()[0]
    grads = {k: v.detach().cpu().clone() for k, v in e.named(e.grad).items()}
    # ... and the sample of step 1 the tail left behind (the nu_omega chain's part 3), at the updated parameters
    par1 = {k: v.detach().cpu().clone() for k, v in e.named().items()}
    omega1 = e.read_site("ω")
    stats = dict(e.stats)
    assert e.status() == (True, -1, 0) and not stats["generic"], stats
    e.close()
    eps = H.philox_eps_list(spec, flat0, SEED, 2)
    H.assert_grads_match_oracle(loss, grads, par0, spec, eps[0])
    rows = H.assert_nuw_rows_match_oracle(grads, par0, spec, eps[0], label)
    om = max(H.assert_omega_matches_oracle(omega0, par0, spec, eps[0], label + " [omega, K_pre]"),
             H.assert_omega_matches_oracle(omega1, par1, spec, eps[1], label + " [omega, chain]"))
    return stats, rows, om


def _structures(case, spec, path, structures, replay, expect):
    """`structures`: {name: tuning}, all bit-identical to the first one; `replay`: the names that run the six-step oracle replay
    themselves (the others are held to it through the bits); expect(name, stats) asserts the path."""
    runs = {}
    for name, tun in structures.items():
        stats, rows, om = _first_step(spec, tun, f"{case} [{path}: {name}]")
        expect(name, stats)
        _note(path, rows, om, spec)
        if name in replay:
            _fused_vs_oracle(spec, n=NSTEPS, seed=SEED, tuning=tun)
        runs[name] = _run(spec, "fused3", NSTEPS, False, seed=SEED, tuning=tun)
    names = list(runs)
    for other in names[1:]:
        _bits_equal(runs[names[0]], runs[other], f"{case}: {names[0]} vs {other}")
    return runs


# ---- the tutorial flow's U-only kernel: per-lane partials in the condition's columns, and the wave reduction ---------------------

PWL_CASES = _select(("vcond", "vcond_mf"), ("tiny_last", "empty_cond"), PWL_SHAPES) + _select(("vcond",), ("tiny_last",), [(2, 1)], Ng=130)


@pytest.mark.parametrize("case", PWL_CASES, ids=str)
def test_per_lane_partials_land_in_their_condition(case):
    spec = _spec(case)
    base = _tuning(case)
    row = 4 if case.Nx * (2 * case.Hw + 1) <= 4 else 8

    def expect(name, stats):
        assert stats["pw_lane"] and stats["pw_inline"] == row and stats["onehot_batches"] == spec.Nb, stats
        assert stats["launches_per_step"] == (3 if name == "three launches" else 2), stats

    _structures(case, spec, "PWL", {"merged tail": base, "tail_merged=False": base.replace(tail_merged=False),
                                    "three launches": base.replace(tail_merged=False, tail2=False)}, {"merged tail"}, expect)


@pytest.mark.parametrize("case", PWL_CASES + _select(("vcond", "vcond_mf"), ("scattered",), PWL_SHAPES), ids=str)
def test_wave_reduction_of_the_u_only_kernel(case):
    """Tuning(pw_lane=False) on the cases above -- and conditions that cut through the batches, where the engine has to decline the
    per-lane partials by itself."""
    spec = _spec(case)
    base = _tuning(case) if case.layout == "scattered" else _tuning(case, pw_lane=False)
    row = 4 if case.Nx * (2 * case.Hw + 1) <= 4 else 8

    def expect(name, stats):
        assert not stats["pw_lane"] and stats["pw_inline"] == row and stats["launches_per_step"] == 2, stats

    structures = {"merged tail": base}
    if case.layout == "scattered":
        structures["tail_merged=False"] = base.replace(tail_merged=False)
    _structures(case, spec, "U-only wave reduction", structures, {"merged tail"}, expect)


# ---- the S+U kernel's own partials ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", _select(("vjoint_h1", "vjoint_lrmn"), ("tiny_last", "scattered"), [(2, 1), (4, 0)]), ids=str)
def test_partials_of_the_s_and_u_kernel(case):
    spec = _spec(case)
    base = _tuning(case, pw_inline="force")
    row = 4 if case.Nx * (2 * case.Hw + 1) <= 4 else 8

    def expect(name, stats):
        assert not stats["pw_lane"] and stats["pw_inline"] == row, stats
        assert stats["launches_per_step"] == (2 if name == "two launches" else 3), stats

    _structures(case, spec, "S+U kernel's partials", {"two launches": base, "three launches": base.replace(tail2=False)},
                {"two launches"}, expect)


# ---- the cell blocks' partials PW -> K_omega -----------------------------------------------------------------------------------------

CELL_BLOCK_CASES = (_select(("vcond", "vjoint_h1", "vjoint_lrmn"), ("tiny_last",), [(2, 1)], orders=("contiguous",))
                    + _select(("vcond", "vjoint_h1", "vjoint_lrmn"), ("tiny_last", "scattered"), [(3, 1), (9, 3)]))


@pytest.mark.parametrize("tail_cells", [256, 1024])
@pytest.mark.parametrize("case", CELL_BLOCK_CASES, ids=str)
def test_cell_block_partials_and_their_column_sums(case, tail_cells):
    """pw_inline="off" -- and 9 and 63 coefficients, more than K_main delivers itself: the third loop of the column sums."""
    spec = _spec(case)
    tun = _tuning(case, pw_inline="off", tail_cells=tail_cells)
    stats, rows, om = _first_step(spec, tun, f"{case} [cell blocks of {tail_cells}]")
    assert stats["launches_per_step"] == 3 and stats["pw_inline"] == 0 and not stats["pw_lane"], stats
    _note(f"cell blocks of {tail_cells} -> PW -> K_omega", rows, om, spec)
    _fused_vs_oracle(spec, n=NSTEPS, seed=SEED, tuning=tun)


# ---- more than 768 partial rows: the column sums leave the registers ---------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in CASES if c.Nc == 3200], ids=str)
def test_more_than_768_partial_rows(case):
    spec = _spec(case)
    vcond = case.model == "vcond"
    base = _tuning(case, cells_per_wave=1, pw_inline=None if vcond else "force")

    def expect(name, stats):
        assert stats["main_grid"] > 768 and stats["pw_inline"] == 8 and stats["pw_lane"] == vcond, stats
        assert stats["launches_per_step"] == (3 if name == "three launches" else 2), stats

    other = {"tail_merged=False": base.replace(tail_merged=False)} if vcond else {}
    _structures(case, spec, "more than 768 partial rows", {"two launches": base, **other,
                                                          "three launches": base.replace(tail_merged=False, tail2=False)}, {"two launches"}, expect)


# ---- the unfused kernels (K_post -> K_fin) and the run-time-sized set: elbo_grad with host draws ------------------------------------

def _unfused(case, tuning, path):
    from velocycle_amd.engine import HipEngine
    p, _ = build(case)
    spec = H.spec_from_problem(p)
    par, eps = point(p, True)
    e = HipEngine(spec, tuning=tuning)
    e.set_params({k: v.float() for k, v in par.items()})
    e.elbo_grad(eps=e.pack_eps({k: v.float() for k, v in eps.items()}))
    torch.cuda.synchronize()
    loss = e.loss()
    grads = {k: v.detach().cpu().clone() for k, v in e.named(e.grad).items()}
    omega = e.read_site("ω")
    stats = dict(e.stats)
    assert e.status() == (True, -1, 0)
    e.close()
    label = f"{case} [{path}]"
    H.assert_grads_match_oracle(loss, grads, par, spec, eps)
    rows = H.assert_nuw_rows_match_oracle(grads, par, spec, eps, label)
    om = H.assert_omega_matches_oracle(omega, par, spec, eps, label)
    _note(path, rows, om, spec)
    return stats


@pytest.mark.parametrize("case", [c for c in CASES if c.Nc == 2100], ids=str)
def test_unfused_kernels_on_three_cell_blocks(case):
    """Nc = 2 100: three 1024-cell blocks of vc_post_cell_block, the last one ragged; conditions 0 / 1 through dx01[], the others
    through another load."""
    stats = _unfused(case, None, "unfused K_post -> K_fin")
    assert not stats["generic"], stats


@pytest.mark.parametrize("case", _select(("vcond", "vjoint_h1", "vjoint_lrmn"), ("tiny_last", "scattered"), [(3, 1)], orders=("contiguous",))
                         + _select(("vjoint_h1",), ("tiny_last", "scattered"), [(2, 4)]), ids=str)
def test_run_time_sized_kernel_set(case):
    from velocycle_amd.tuning import Tuning
    stats = _unfused(case, None if case.Hw == 4 else Tuning(force_generic=True), "run-time-sized set")
    assert stats["generic"], stats


# ---- sharded: phases A / B of three ranks on one device (tests/test_hip_sharded_step.py) --------------------------------------------

@pytest.mark.parametrize("case", _select(("vcond", "vjoint_h1"), ("tiny_last",), [(3, 1)]), ids=str)
def test_sharded_step_holds_every_condition_row(case):
    """world = 3.  Contiguous cells: rank 0 holds cells of condition 0 only, the tiny condition lives on one rank; interleaved: every
    rank holds some of every condition.  The summed gradient of the first step (left in `grad` by phase B; phi_xy blocks concatenated
    over the ranks) and omega of every rank's cells against the oracle, six steps against the oracle replay, replicated state
    bit-identical on the ranks."""
    from velocycle_amd.engine import HipEngine
    from tests.test_hip_batch_paths import _sharded_state
    from tests.test_hip_sharded_step import _Rank, _run_sharded, OPT as SOPT
    spec = _spec(case)
    tun = _tuning(case, cells_per_wave=1)
    world, n, seed = 3, NSTEPS, 5
    nz = lambda t: torch.nan_to_num(t, neginf=-1e30)
    probe = [_Rank(spec, r, world, seed, tun) for r in range(world)]
    par0 = _sharded_state(probe)
    for r in probe:
        r.e.close()
    e0 = HipEngine(spec)
    e0.set_params(par0)
    flat0 = e0.params.detach().clone()
    e0.close()
    eps = H.philox_eps_list(spec, flat0, seed, n)
    ranks = _run_sharded(spec, world, 1, seed, tun)
    grads = {k: v.detach().cpu().clone() for k, v in ranks[0].e.named(ranks[0].e.grad).items()}
    grads["ϕxy_locs"] = torch.cat([r.e.view(r.e.grad, "ϕxy_locs").detach().cpu() for r in ranks])
    par1 = _sharded_state(ranks)
    omega1 = torch.cat([r.e.read_site("ω") for r in ranks])
    loss = float(ranks[0].ring[0].item())
    cond = spec.D.argmax(0)
    held = [sorted(set(cond[r.e.c0:r.e.c1].tolist())) for r in ranks]
    if case.order == "contiguous":
        assert held[0] == [0] and sum(spec.Nx - 1 in h for h in held) == 1, held
    for r in ranks:
        assert r.e.status() == (True, -1, 0) and r.e.stats["pw_inline"] == 0
        r.e.close()
    label = f"sharded {case}"
    H.assert_grads_match_oracle(loss, grads, par0, spec, eps[0])
    rows = H.assert_nuw_rows_match_oracle(grads, par0, spec, eps[0], label)
    om = H.assert_omega_matches_oracle(omega1, par1, spec, eps[1], label)
    _note("sharded phases A / B", rows, om, spec)
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


# ---- K particles ---------------------------------------------------------------------------------------------------------------------

def test_particle_step_with_a_tiny_condition():
    """SVIRunner(num_particles=3), eight steps on the three-cell condition: the kernels compiled for the configuration's signature
    against the run-time-flag kernels (Tuning(no_tail_spec=True)) and the C call against the host loop of K x vc_elbo_grad
    (Tuning(particles_host_loop=True)), as tests/test_hip_batch_paths.py::test_particle_step_with_many_batches: bit for bit."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    case = Case("vjoint_h1", "tiny_last", "contiguous", 3, 1, 800, 70)
    assert case in CASES
    spec, tun = _spec(case), _tuning(case)
    out = []
    for t in (tun, tun.replace(no_tail_spec=True), tun.replace(particles_host_loop=True)):
        e = HipEngine(spec, tuning=t)
        if t.no_tail_spec:
            assert e.stats["tail_spec_name"] == "generic"
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
