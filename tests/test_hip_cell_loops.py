"""GPU: the likelihood kernel's long cell loops held to the float64 oracle cell by cell.

vc_main_kernel walks `cw` consecutive cells per wave: PF + 1 rotating register buffers whose tail re-fetches the last cell, the
16-cell LDS tile of the S+U kernel (flushed at (i & 15) == 15), the 64-cell staging of the one-sum kernels (flushed at
(i & 63) == 63 and then continued into the same staging lanes), the per-lane accumulators of the PWL instantiation, and waves
without any cell that still drain their early fetches.  The engine's own tiling gives 8 cells per wave at every size the suite
builds, and in the U-only kernels (the tutorials' velocity stage) a cell reaches nothing but gene-level sums and the nu_omega
partials: on ordinary counts one wrong cell lies at or under the block-wise bar (tests/test_cell_rows_cpu.py).

Here every kernel family runs ONE evaluation per case on lit-cell probe data (helpers.lit_cell_problem: every cell lit in one gene
per matrix, every gene in m <= 17 cells, no element near the relu kink) with Tuning(cells_per_wave=cw),
cw in {1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 130}, Nc = 4 cw n_wg + cw + 1 -- the last workgroup has a full wave, a wave with a single
cell and two waves with none.  Asserted per case: the instantiation that ran and the tiling (engine.stats), the loss and every block
at assert_grads_match_oracle's bars, every gene row -- and every cell's row where phi_xy is learned -- within 2e-3 of its OWN
max-norm (helpers.assert_gene_rows_match_oracle), the nu_omega rows per condition (helpers.assert_nuw_rows_match_oracle), and, as a
condition on the inputs, the float32 oracle's own rows within 0.25 of that bar at the very point and draws of the evaluation.

Two ways to an evaluation.  "fused": the first step of SVIRunner's fused perf step from the initial parameters with the Philox
draws, read from the gradient buffer (tests/test_hip_nuw_paths.py::_first_step; elbo_grad launches the row-storing twin of the PWL
instantiation); with loss_every = 2 the SECOND step, which runs the gradient-only twin and forms no loss.  "unfused": elbo_grad with
host draws at tests/test_cell_rows_cpu.py::point's perturbed parameters.

Measured on an MI355X, worst gene-row err / bar over all cw (printed per case by -s; DESIGN section 4 has every family): U-only NB 0.060
(PWL and wave reduction alike), their gradient-only twins 0.132, Poisson 0.092, Lognormal 0.061; phase < 1e-3 (cell rows 0.004); S+U
0.053 (cell rows 0.049); two gene blocks 0.248 (`rho_real_loc`, the float32 oracle itself at 0.15); nu_omega rows <= 3e-4.  The
worst rows are the LRMN guide's `cov_diag` / `rho_real_loc` entries, where the float32 oracle's own error is largest too.  No kernel
bug was found; what five deliberately wrong builds of the loop showed is in DESIGN section 4."""
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_cell_rows_cpu as T
from tests.test_cell_rows_cpu import CWS, F32_BAR, SHAPES, TWO_BATCH_SIZES, probe_cells

pytestmark = pytest.mark.gpu

OPT = {"lr": 0.03, "lrd": 0.995, "betas": (0.8, 0.99)}
SEED = 3
# The Philox seed of a fused case is SEED -- except where those draws violate the condition on the inputs asserted in _held (the
# float32 ORACLE's own rows within F32_BAR of the per-gene bar): then another seed, never another number.
# {(model, Nc, Ng, gradient-only twin): seed}.  vcond at 698 cells, step 1 of seed 3: a `cov_diag` row of log gamma whose likelihood and
# entropy parts cancel leaves the float32 oracle at 0.385 of that row's bar
FUSED_SEEDS = {("vcond", 698, 70, True): 4}
WORST = {}          # family -> [worst gene row, worst cell row, worst nu_omega row] err / bar so far


def _tuning(cw, gpl=0, **kw):
    from velocycle_amd.tuning import Tuning
    return Tuning(cells_per_wave=cw, genes_per_lane=gpl, **kw)


def _spec(model, Nc, Ng):
    return H.spec_from_problem(T.build(model, Nc, Ng))


def _tiling(stats, cw, Nc, Ng, gpl=None, waves=4):
    """Tuning(cells_per_wave=cw) was honoured: every pass at cw cells per wave, ceil(Nc / (waves cw)) workgroups per gene block."""
    assert stats["pass_cells"] == [cw] * 4, stats
    if gpl:
        assert f"gpl{gpl}" in stats["main_kernel"], stats
        assert stats["main_grid"] == -(-Ng // (64 * gpl)) * -(-Nc // (waves * cw)), stats


def _held(family, case, loss, grads, par, spec, eps):
    """The numerical assertions of one evaluation; prints the case's and the family's running worst err / bar."""
    label = f"{family} {case}"
    p64 = H.problem_from_spec(spec, torch.float64)
    par64 = {k: v.detach().cpu().double() for k, v in par.items()}
    e64 = {k: v.detach().cpu().double() for k, v in eps.items() if not k.startswith("_")}
    f32 = T._float32_rows(p64, par64, e64)
    assert max(f32.values()) <= F32_BAR, ("condition on the inputs, not on the kernels: choose another seed for this case", label, f32)
    H.assert_grads_match_oracle(loss, grads, par, spec, eps)
    rows = H.assert_gene_rows_match_oracle(grads, par, spec, eps, label)
    cell = rows.pop("ϕxy_locs", 0.0)
    nuw = 0.0
    if spec.kind == "velocity" and "νω" not in spec.condition_on:
        nuw = max(float(np.nanmax(v)) for v in H.assert_nuw_rows_match_oracle(grads, par, spec, eps, label).values())
    gene = max(rows.values())
    w = WORST.setdefault(family, [0.0, 0.0, 0.0])
    w[:] = [max(w[0], gene), max(w[1], cell), max(w[2], nuw)]
    print(f"[cell loops] {label}: gene rows {gene:.2e} ({max(rows, key=rows.get)}), cell rows {cell:.2e}, nu_omega rows {nuw:.2e}, float32 "
          f"oracle {max(f32.values()):.2e} of the bar; {family} so far: {w[0]:.2e} / {w[1]:.2e} / {w[2]:.2e}")


def _fused(family, model, Nc, Ng, tuning, twin=False):
    """The first fused step (twin: the second, by the gradient-only kernel).  Returns the engine's stats."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.svi import SVIRunner
    assert (model, Nc, Ng) in {(m, n, g) for m, _, n, g in SHAPES}          # tests/test_cell_rows_cpu.py holds the conditions on it
    spec = _spec(model, Nc, Ng)
    seed = FUSED_SEEDS.get((model, Nc, Ng, twin), SEED)
    e = HipEngine(spec, tuning=tuning)
    try:
        try:
            r = SVIRunner(e, OPT, mode="perf", seed=seed, loss_every=2 if twin else 1)
        except NotImplementedError as exc:
            pytest.skip(f"no gradient-only twin of {e.stats['main_kernel']}: {exc}")
        assert r.adam_impl == "fused3" and not r.use_graph
        flat0 = e.params.detach().clone()
        par = {k: v.detach().cpu().clone() for k, v in e.named().items()}
        r.run_perf(1)
        step = 0
        if twin:
            # step 1 starts from what step 0 left and runs the gradient-only kernel: its gradient is what the buffer holds afterwards
            par = {k: v.detach().cpu().clone() for k, v in e.named().items()}
            r.run_perf(1)
            step = 1
        losses = r.perf_losses()
        grads = {k: v.detach().cpu().clone() for k, v in e.named(e.grad).items()}
        stats = dict(e.stats)
        assert e.status() == (True, -1, 0), e.status()
    finally:
        e.close()
    eps = H.philox_eps_list(spec, flat0, seed, step + 1)
    if twin:
        assert math.isfinite(losses[0]) and math.isnan(losses[1]), losses
    _held(family, f"{model} cw={tuning.cells_per_wave} {Nc}x{Ng}", None if twin else losses[0], grads, par, spec, eps[step])
    return stats


def _unfused(family, model, Nc, Ng, tuning):
    from velocycle_amd.engine import HipEngine
    assert (model, Nc, Ng) in {(m, n, g) for m, _, n, g in SHAPES}
    p, par, eps = T.point_of(model, Nc, Ng, True)
    spec = H.spec_from_problem(p)
    e = HipEngine(spec, tuning=tuning)
    try:
        e.set_params({k: v.float() for k, v in par.items()})
        e.elbo_grad(eps=e.pack_eps({k: v.float() for k, v in eps.items()}))
        torch.cuda.synchronize()
        loss = e.loss()
        grads = {k: v.detach().cpu().clone() for k, v in e.named(e.grad).items()}
        stats = dict(e.stats)
        assert e.status() == (True, -1, 0), e.status()
    finally:
        e.close()
    _held(family, f"{model} cw={tuning.cells_per_wave} {Nc}x{Ng}", loss, grads, par, spec, eps)
    return stats


def _u_only(stats, noise="nb", pwl=False, storage="u16"):
    k = stats["main_kernel"]
    assert not stats["generic"] and f"vu_{noise}" in k and stats["pw_lane"] == pwl and (",pwl" in k) == pwl, stats
    assert stats["count_storage"] == storage and (",u16" in k) == (storage == "u16"), stats


# ---- U-only negative binomial: the PWL instantiation (the tutorial stage's default) ------------------------------------------------

PWL_CONFIGS = [(cw, model, storage, gpl) for model in ("vcond", "vcond_mf_hw0") for storage in ("u16", "f32") for gpl in (8, 4) for cw in CWS]


@pytest.mark.parametrize("cw,model,storage,gpl", PWL_CONFIGS)
def test_per_lane_instantiation(cw, model, storage, gpl):
    """H omega = 1 (vcond, LRMN) and 0 (vcond_mf_hw0, mean-field); uint16 and float32 counts; 4 and 8 genes per lane."""
    Nc = probe_cells(cw)
    stats = _fused("U-only NB, PWL", model, Nc, 70, _tuning(cw, gpl, count_storage="f32" if storage == "f32" else None))
    _u_only(stats, pwl=True, storage=storage)
    assert stats["pw_inline"] == 4 and stats["launches_per_step"] == 2, stats
    _tiling(stats, cw, Nc, 70, gpl)


@pytest.mark.parametrize("cw,model,storage,gpl", [(cw, "vcond", "u16", 8) for cw in CWS] + [(cw, "vcond_mf_hw0", "f32", 4) for cw in (3, 17, 65, 130)])
def test_per_lane_instantiation_gradient_only_twin(cw, model, storage, gpl):
    Nc = probe_cells(cw)
    stats = _fused("U-only NB, PWL, gradient-only", model, Nc, 70, _tuning(cw, gpl, count_storage="f32" if storage == "f32" else None), twin=True)
    _u_only(stats, pwl=True, storage=storage)
    _tiling(stats, cw, Nc, 70, gpl)


# ---- U-only negative binomial with the wave reduction: the 64-cell staging; the kernel the sharded phases launch ---------------------

@pytest.mark.parametrize("pw_inline", [None, "off"])
@pytest.mark.parametrize("cw", CWS)
def test_wave_reduction(cw, pw_inline):
    """pw_inline auto: K_main's own nu_omega partials, formed at the flush of the staged sums; "off": the per-cell rows alone."""
    Nc = probe_cells(cw)
    stats = _fused(f"U-only NB, wave reduction, pw_inline {pw_inline or 'auto'}", "vcond", Nc, 70, _tuning(cw, 8, pw_lane=False, pw_inline=pw_inline))
    _u_only(stats)
    assert stats["pw_inline"] == (0 if pw_inline == "off" else 4) and stats["launches_per_step"] == (3 if pw_inline == "off" else 2), stats
    _tiling(stats, cw, Nc, 70, 8)


@pytest.mark.parametrize("cw", CWS)
def test_wave_reduction_gradient_only_twin(cw):
    Nc = probe_cells(cw)
    stats = _fused("U-only NB, wave reduction, gradient-only", "vcond", Nc, 70, _tuning(cw, 8, pw_lane=False), twin=True)
    _u_only(stats)
    _tiling(stats, cw, Nc, 70, 8)


# ---- U-only Poisson and Lognormal ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", ["poisson", "lognormal"])
@pytest.mark.parametrize("cw", CWS)
def test_u_only_poisson_and_lognormal(cw, noise):
    Nc = probe_cells(cw)
    stats = _unfused(f"U-only {noise}", f"vcond_{noise}", Nc, 70, _tuning(cw))
    _u_only(stats, noise=noise, storage="f32" if noise == "lognormal" else "u16")
    _tiling(stats, cw, Nc, 70)


# ---- phase: the staging path with phi_xy learned -- rows per cell as well -------------------------------------------------------------

@pytest.mark.parametrize("noise", ["nb", "poisson", "lognormal"])
@pytest.mark.parametrize("cw", CWS)
def test_phase_kernels(cw, noise):
    Nc = probe_cells(cw)
    stats = _unfused(f"phase {noise}", f"phase_{noise}", Nc, 70, _tuning(cw))
    assert not stats["generic"] and f"phase_{noise}" in stats["main_kernel"], stats
    _tiling(stats, cw, Nc, 70)


@pytest.mark.parametrize("cw", (3, 16, 17, 64, 65, 130))
def test_phase_gradient_only_twin(cw):
    Nc = probe_cells(cw)
    stats = _fused("phase NB, gradient-only", "phase_nb", Nc, 70, _tuning(cw), twin=True)
    assert not stats["generic"] and "phase_nb" in stats["main_kernel"], stats
    _tiling(stats, cw, Nc, 70)


# ---- S+U negative binomial: the 16-cell LDS tile; cw >= 63 is new ---------------------------------------------------------------------

@pytest.mark.parametrize("model", ["vjoint", "vjoint_lrmn"])
@pytest.mark.parametrize("cw", CWS)
def test_s_and_u_kernel(cw, model):
    """Mean-field: the fused step with K_main's own nu_omega partials forced (formed at the tile flush, accumulators in the LDS) --
    declined by the engine itself where the W rows of cw cells do not fit, which the case prints; LRMN: elbo_grad."""
    Nc = probe_cells(cw)
    if model == "vjoint":
        stats = _fused("S+U NB mean-field", model, Nc, 70, _tuning(cw, pw_inline="force"))
        print(f"[cell loops] S+U mean-field cw={cw}: pw_inline {stats['pw_inline']}, {stats['launches_per_step']} launches per step")
    else:
        stats = _unfused("S+U NB LRMN", model, Nc, 70, _tuning(cw))
    assert not stats["generic"] and "vfull_nb" in stats["main_kernel"] and not stats["pw_lane"], stats
    _tiling(stats, cw, Nc, 70)


@pytest.mark.parametrize("cw", (3, 16, 17, 64, 65, 130))
def test_s_and_u_gradient_only_twin(cw):
    Nc = probe_cells(cw)
    stats = _fused("S+U NB, gradient-only", "vjoint", Nc, 70, _tuning(cw), twin=True)
    assert not stats["generic"] and "vfull_nb" in stats["main_kernel"], stats
    _tiling(stats, cw, Nc, 70)


# ---- two and three harmonics ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["vcond_h2", "vcond_h3", "phase_h2", "phase_h3", "vjoint_h2", "vjoint_h3"])
@pytest.mark.parametrize("cw", (17, 65))
def test_two_and_three_harmonics(cw, model):
    Nc = probe_cells(cw)
    Hh = T.MODELS[model][3]
    if model.startswith("vcond"):
        # H = 2: the PWL instantiation; H = 3: the wave reduction
        pwl = Hh == 2
        stats = _fused(f"U-only NB, H = {Hh}", model, Nc, 70, _tuning(cw, pw_lane=pwl))
        _u_only(stats, pwl=pwl)
    else:
        stats = _unfused(f"{'phase' if model.startswith('phase') else 'S+U'} NB, H = {Hh}", model, Nc, 70, _tuning(cw))
        assert not stats["generic"] and ("phase_nb" if model.startswith("phase") else "vfull_nb") in stats["main_kernel"], stats
    assert stats["main_kernel"].startswith(f"vc_main_kernel<{Hh},0,"), stats
    _tiling(stats, cw, Nc, 70)


# ---- two gene blocks: 300 genes at four genes per lane -------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["vcond", "vcond_mf_hw0", "vjoint", "vjoint_lrmn", "phase_nb"])
def test_two_gene_blocks(model):
    cw, Nc = 130, probe_cells(130)
    if model.startswith("vcond"):
        pwl = model == "vcond"
        stats = _fused("two gene blocks", model, Nc, 300, _tuning(cw, 4, pw_lane=pwl))
        _u_only(stats, pwl=pwl)
    else:
        stats = _unfused("two gene blocks", model, Nc, 300, _tuning(cw, 4))
    _tiling(stats, cw, Nc, 300, 4)
    assert stats["main_grid"] == 2 * 3, stats


# ---- two one-hot batches with two conditions: batch-aligned workgroups from vc_tile_batches --------------------------------------------

def test_two_batches_with_two_conditions():
    """780 + 257 cells at 65 cells per wave: vc_tile_batches gives batch 0 three workgroups of 4 x 65 cells and batch 1 one of
    65, 65, 65, 62; each workgroup's per-lane partials go to the columns of its batch's condition."""
    Nc = sum(TWO_BATCH_SIZES)
    stats = _fused("two batches, two conditions", "vcond_2b", Nc, 70, _tuning(65, 8))
    _u_only(stats, pwl=True)
    assert stats["onehot_batches"] == 2 and stats["pw_inline"] == 8 and stats["main_grid"] == 4 and stats["pass_cells"] == [65] * 4, stats


# ---- the run-time-sized kernel set --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cw", (1, 17, 65))
def test_run_time_sized_set(cw):
    """Tuning(force_generic=True) honours cells_per_wave, with ONE wave per workgroup (vc_engine.hip: the tile table is built for
    `d.generic ? 1 : VC_WAVES` waves): ceil(Nc / cw) workgroups per gene block, the last one with the probe's single left-over cell."""
    from velocycle_amd.tuning import Tuning
    Nc = probe_cells(cw)
    stats = _unfused("run-time-sized set", "vcond", Nc, 70, Tuning(force_generic=True, cells_per_wave=cw))
    assert stats["generic"] and "generic_vu" in stats["main_kernel"], stats
    assert stats["pass_cells"] == [cw] * 4 and stats["main_grid"] % -(-Nc // cw) == 0, stats
