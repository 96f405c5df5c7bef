"""CPU: the lit-cell probe and the power of the per-gene comparator (tests/helpers.py: lit_cell_problem,
assert_gene_rows_match_oracle), on the oracle alone.

Every gene-level gradient of the likelihood kernel is a sum over all cells, and in the U-only kernels (phi_xy, nu and shape_inv
conditioned: the tutorials' velocity stage) a cell reaches nothing but those sums and the nu_omega partials.  On the suite's random
counts one cell among a few thousand moves the worst gene row by about one bar of the block-wise 2e-3 max-norm bar: a cell left
out, counted twice or evaluated with its neighbour's record at some residue of the cell loop passes.  This file owns the table of
models and shapes tests/test_hip_cell_loops.py runs (MODELS, probe_cells, SHAPES / build) and asserts on every entry, with the faults
planted on the ORACLE side at the cells where the kernel's loop changes shape (first and last cell, both sides of a wave range
boundary, in-range positions 15 / 16 and 63 / 64):

  * the float32 oracle's own worst row is <= F32_BAR = 0.25 of the per-gene bar in every block (per cell for a learned phi_xy);
  * (a) one cell left out and (b) one cell counted twice move at least one gene row by >= DROP_BARS = 5 bars at every planted cell;
  * (c) two neighbouring cells' counts exchanged (a cell evaluated with its neighbour's record) move one by >= SWAP_BARS = 3 bars;
  * the same faults on `_problem`'s ordinary random counts stay under BLIND_BARS = 2 bars of the BLOCK-wise bar from 2 100 cells up --
    the blind spot, recorded.  (Not at the probe's own 402 .. 1 171 cells: one cell is 1 / Nc of a row, and there ordinary counts show
    a dropped cell at 1.1 - 5.3 block bars; test_the_block_bar_does_not_see_one_cell_of_ordinary_counts prints those and says why.)

Measured (float64 oracle; the worst over the 117 table entries, both evaluation points and every planted cell; printed by -s):
float32 oracle 0.185 of the bar (`cov_diag` of log gamma, LRMN; 0.29 - 0.39 where a scale-type row's likelihood and entropy parts
cancel: those four entries draw from another seed, DRAW_SEEDS); negative binomial and Poisson: left out / twice 29 - 127 bars
(~500 / m), exchanged 6.1 (U-only, H = 3) - 184; Lognormal: left out / twice 6.6 (phase, 1 106 cells), exchanged 5.4 (U-only,
1 072 cells).  Ordinary counts at 2 100 / 3 000 x 70: left out 0.7 - 1.6 block bars."""
import functools

import numpy as np
import pytest
import torch

from oracle import velocycle_oracle as orc
from tests import helpers as H
from tests.test_hip_sweep import _problem

F32_BAR, DROP_BARS, SWAP_BARS, BLIND_BARS = 0.25, 5.0, 3.0, 2.0

CWS = (1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 130)
_N_WG = {1: 100, 2: 60, 3: 40, 5: 30, 15: 10, 16: 10, 17: 10, 63: 4, 64: 4, 65: 4, 130: 2}


def probe_cells(cw):
    """Nc = 4 cw n_wg + cw + 1: n_wg full workgroups of four waves, then one with a full wave, a wave with a single cell and two
    waves with none.  402 .. 1 171 cells: every gene of 70 is lit in m <= 17 cells."""
    return 4 * cw * _N_WG[cw] + cw + 1


VU, VU_NO_SI = ["ϕxy", "ν", "shape_inv"], ["ϕxy", "ν"]
#          kind, guide, noise, H, Hw, Nb, Nx, conditioned sites
MODELS = {"vcond": ("velocity", "lrmn", "NegativeBinomial", 1, 1, 0, 1, VU),              # the tutorials' velocity stage
          "vcond_mf_hw0": ("velocity", "meanfield", "NegativeBinomial", 1, 0, 0, 1, VU),
          "vcond_poisson": ("velocity", "lrmn", "Poisson", 1, 1, 0, 1, VU_NO_SI),
          "vcond_lognormal": ("velocity", "meanfield", "Lognormal", 1, 1, 0, 1, VU_NO_SI),
          "vcond_h2": ("velocity", "lrmn", "NegativeBinomial", 2, 1, 0, 1, VU),
          "vcond_h3": ("velocity", "meanfield", "NegativeBinomial", 3, 1, 0, 1, VU),
          "vcond_2b": ("velocity", "lrmn", "NegativeBinomial", 1, 1, 2, 2, VU + ["Δν"]),    # two one-hot batches = two conditions
          "phase_nb": ("phase", "meanfield", "NegativeBinomial", 1, 0, 0, 0, []),
          "phase_poisson": ("phase", "meanfield", "Poisson", 1, 0, 0, 0, []),
          "phase_lognormal": ("phase", "meanfield", "Lognormal", 1, 0, 0, 0, []),
          "phase_h2": ("phase", "meanfield", "NegativeBinomial", 2, 0, 0, 0, []),
          "phase_h3": ("phase", "meanfield", "NegativeBinomial", 3, 0, 0, 0, []),
          "vjoint": ("velocity", "meanfield", "NegativeBinomial", 1, 1, 0, 1, []),
          "vjoint_lrmn": ("velocity", "lrmn", "NegativeBinomial", 1, 1, 0, 1, []),
          "vjoint_h2": ("velocity", "meanfield", "NegativeBinomial", 2, 1, 0, 1, []),
          "vjoint_h3": ("velocity", "lrmn", "NegativeBinomial", 3, 1, 0, 1, [])}
TWO_BATCH_SIZES = (780, 257)       # vcond_2b at 65 cells per wave: three full workgroups for batch 0; 65, 65, 65, 62 cells for batch 1


def _shapes():
    """(model, cells per wave, Nc, Ng) of every problem the GPU file evaluates."""
    out = []
    for m in ("vcond", "vcond_mf_hw0", "vcond_poisson", "vcond_lognormal", "phase_nb", "phase_poisson", "phase_lognormal", "vjoint",
              "vjoint_lrmn"):
        out += [(m, cw, probe_cells(cw), 70) for cw in CWS]
    for m in ("vcond_h2", "vcond_h3", "phase_h2", "phase_h3", "vjoint_h2", "vjoint_h3"):
        out += [(m, cw, probe_cells(cw), 70) for cw in (17, 65)]
    out += [(m, 130, probe_cells(130), 300) for m in ("vcond", "vcond_mf_hw0", "vjoint", "vjoint_lrmn", "phase_nb")]
    out.append(("vcond_2b", 65, sum(TWO_BATCH_SIZES), 70))
    return out


SHAPES = _shapes()
# The host draws of a shape come from seed 1 -- except where that draw violates a condition asserted below (a `rho_real_loc` or
# `cov_diag` row whose likelihood and entropy parts cancel so far that the float32 oracle's own rounding is 0.29 - 0.35 of the row's
# bar): then another seed, never another number.  {(model, Nc, Ng): seed}
DRAW_SEEDS = {("vcond", 657, 70): 2, ("vcond_poisson", 657, 70): 2, ("vjoint_lrmn", 657, 70): 2, ("vjoint_h3", 1106, 70): 2}


@functools.lru_cache(maxsize=None)
def build(model, Nc, Ng, lit=True):
    """The float64 oracle Problem: `_problem`'s data (seed from the shape), as a lit-cell probe unless lit=False."""
    kind, guide, noise, Hh, Hw, Nb, Nx, sites = MODELS[model]
    p = _problem(kind, guide, noise, Hh, Hw, Nb, Nx, sites, Nc=Nc, Ng=Ng, seed=12000 + 7 * Nc + Ng + sorted(MODELS).index(model))
    if model == "vcond_2b":
        assert Nc == sum(TWO_BATCH_SIZES)
        ids = torch.cat([torch.full((n,), q, dtype=torch.long) for q, n in enumerate(TWO_BATCH_SIZES)])
        p.Db = H.onehot_Db(ids, 2)
        p.D = H.onehot_Db(ids, 2)
    return H.lit_cell_problem(p) if lit else p


def point(p, perturbed, seed=1):
    """(parameters, draws), float32 values held in float64: the guide's initial parameters (where the first fused step evaluates,
    there with the device's own draws), or those + 0.01 x noise (what the unfused GPU cases evaluate: off the prior means, and the
    harmonics of nu still where lit_cell_problem put them -- the sweep's 0.05 on three harmonics moves z by up to 0.3)."""
    gen = torch.Generator().manual_seed(seed)
    first = orc.draw_eps(p, gen)
    eps = orc.draw_eps(p, gen)
    par = orc.init_params(p, first.get("_cov_factor_draw"))
    if perturbed:
        for k in par:
            if torch.isfinite(par[k]).all():
                par[k] = par[k] + 0.01 * torch.randn(par[k].shape, generator=gen, dtype=torch.float64)
    return ({k: v.float().double() for k, v in par.items()},
            {k: v.float().double() for k, v in eps.items() if not k.startswith("_")})


def point_of(model, Nc, Ng, perturbed, lit=True):
    """(problem, parameters, draws) of a table entry, with the entry's draw seed."""
    p = build(model, Nc, Ng, lit)
    return (p,) + point(p, perturbed, DRAW_SEEDS.get((model, Nc, Ng), 1))


def planted_cells(cw, Nc):
    """The cells a fault is planted at: first, last; k cw - 1 and k cw (the last cell of a wave's range and the first of the next:
    k = 5, the second workgroup's first two waves); in-range positions 15 / 16 and 63 / 64 of the range that starts at 2 cw."""
    cells = {0, Nc - 1, 5 * cw - 1, 5 * cw}
    if cw > 16:
        cells |= {2 * cw + 15, 2 * cw + 16}
    if cw > 64:
        cells |= {2 * cw + 63, 2 * cw + 64}
    return sorted(c for c in cells if 0 <= c < Nc)


_CELL_FIELDS = ("S", "U", "count_factor", "phixy_prior")


def without_cell(p, par, eps, c):
    """(problem, parameters, draws) with cell c removed altogether."""
    keep = torch.arange(p.Nc) != c
    kw = dict(p.__dict__)
    for f in _CELL_FIELDS:
        if kw.get(f) is not None:
            kw[f] = kw[f][..., keep] if f in ("S", "U") else kw[f][keep]
    kw["Db"] = p.Db[:, keep]
    if p.D is not None:
        kw["D"] = p.D[:, keep]
    kw["condition_on"] = {k: (v.reshape(p.Nc, 2)[keep] if k == "ϕxy" else v) for k, v in p.condition_on.items()}
    par = {k: (v[keep] if k == "ϕxy_locs" else v) for k, v in par.items()}
    eps = {k: (v.reshape(p.Nc, 2)[keep] if k == "ϕxy" else v) for k, v in eps.items()}
    return orc.Problem(**kw), par, eps


def exchanged(p, c):
    """The counts of cell c and its neighbour (c + 1; c - 1 for the last cell) exchanged, everything else of the two cells in place."""
    o = c + 1 if c + 1 < p.Nc else c - 1
    kw = dict(p.__dict__)
    for f in ("S", "U"):
        if kw.get(f) is not None:
            M = kw[f].clone()
            M[:, [c, o]] = M[:, [o, c]]
            kw[f] = M
    return orc.Problem(**kw)


def _gene_blocks(g, p):
    b = H.gene_row_blocks(g, p)
    b.pop("ϕxy_locs", None)
    return b


def _faults(p, par, eps, cells):
    """{cell: {"a" | "b" | "c": (worst err / per-gene bar, worst err / block-wise bar)}} on the gene-indexed blocks."""
    _, g, _, _ = orc.loss_and_grads(p, par, eps)
    want = _gene_blocks(g, p)
    block_bar = {k: H.GENE_ROW_RTOL * max(float(H._rowmax(v).max()), H.GENE_ROW_FLOOR) for k, v in want.items()}

    def score(got):
        rows = max(float(v.max()) for v in H.gene_row_ratios(got, want).values())
        blk = max(float(H._rowmax(got[k] - want[k]).max()) / block_bar[k] for k in want)
        return rows, blk

    out = {}
    for c in cells:
        ga = _gene_blocks(orc.loss_and_grads(*without_cell(p, par, eps, c))[1], p)
        gb = {k: 2.0 * want[k] - ga[k] for k in want}          # the sums are linear in the cells: one more = twice the sum minus one less
        gc = _gene_blocks(orc.loss_and_grads(exchanged(p, c), par, eps)[1], p)
        out[c] = {"a": score(ga), "b": score(gb), "c": score(gc)}
    return out


def _float32_rows(p, par, eps):
    _, g64, _, _ = orc.loss_and_grads(p, par, eps)
    _, g32, _, _ = orc.loss_and_grads(p.to(torch.float32), {k: v.float() for k, v in par.items()}, {k: v.float() for k, v in eps.items()})
    out = {k: float(v.max()) for k, v in H.gene_row_ratios(H.gene_row_blocks(g32, p), H.gene_row_blocks(g64, p)).items()}
    if p.kind == "velocity" and "νω" not in p.condition_on:
        # ... and the nu_omega rows against helpers.assert_nuw_rows_match_oracle's bar, which the GPU cases hold beside the gene rows
        want, _, _, bar = H.nuw_row_bars(par, p, eps)
        got = H.nuw_row_blocks(g32, p)
        out.update({k: float((H._rowmax(got[k] - want[k]) / bar[k]).max()) for k in want})
    return out


def test_the_probe_is_what_the_gpu_tests_rely_on():
    assert [probe_cells(cw) for cw in CWS] == [402, 483, 484, 606, 616, 657, 698, 1072, 1089, 1106, 1171]
    p = build("vcond", probe_cells(17), 70)
    assert p.Nc == 698 and float(p.S.sum()) == float(p.U.sum()) == 698 * H.LIT_COUNT
    assert bool(((p.S > 0).sum(0) == 1).all()) and bool(((p.U > 0).sum(0) == 1).all())
    lit = (p.S > 0).sum(1)
    assert int(lit.min()) == 9 and int(lit.max()) == 10                                   # m = Nc / Ng, <= 50
    assert torch.equal(torch.nonzero(p.S[:, 71]).reshape(-1), torch.tensor([1])) and torch.equal(torch.nonzero(p.U[:, 71]).reshape(-1), torch.tensor([2]))
    assert float(p.S.max()) == H.LIT_COUNT < 2048 and abs(float(p.mu_nu[:, 0].mean()) - H.LIT_LEVEL) < 0.1
    for model, cw, Nc, Ng in SHAPES:
        assert Nc / Ng <= 50 and 400 <= Nc <= 1200
    assert planted_cells(130, 1171) == [0, 275, 276, 323, 324, 649, 650, 1170]
    assert planted_cells(16, 657) == [0, 79, 80, 656]
    # removing a cell removes it everywhere; exchanging moves the counts alone
    par, eps = point(p, False)
    q, par1, eps1 = without_cell(p, par, eps, 5)
    assert q.Nc == 697 and torch.equal(q.S[:, 5], p.S[:, 6]) and torch.equal(q.condition_on["ϕxy"][5], p.condition_on["ϕxy"].reshape(-1, 2)[6])
    x = exchanged(p, 697)
    assert torch.equal(x.U[:, 697], p.U[:, 696]) and torch.equal(x.U[:, 696], p.U[:, 697]) and x.count_factor is p.count_factor


@pytest.mark.parametrize("model,cw,Nc,Ng", SHAPES, ids=lambda v: str(v))
def test_the_per_gene_bar_sees_one_cell(model, cw, Nc, Ng):
    worst32 = {}
    for perturbed in (False, True):           # the first fused step's point, and the unfused evaluations' perturbed point
        p, par, eps = point_of(model, Nc, Ng, perturbed)
        if p.kind == "velocity":
            assert H.lit_z_min(p, par, eps) >= H.LIT_Z_MIN
        for k, v in _float32_rows(p, par, eps).items():
            worst32[k] = max(worst32.get(k, 0.0), v)
    p, par, eps = point_of(model, Nc, Ng, False)
    f = _faults(p, par, eps, planted_cells(cw, Nc))
    low = {n: min(v[n][0] for v in f.values()) for n in "abc"}
    print(f"[cell rows] {model} cw={cw} {Nc}x{Ng}: float32 oracle / bar {max(worst32.values()):.3f} ({max(worst32, key=worst32.get)}); weakest planted "
          f"fault, bars: left out {low['a']:.1f}, twice {low['b']:.1f}, exchanged {low['c']:.1f}")
    assert max(worst32.values()) <= F32_BAR, (model, worst32)
    for c, v in f.items():
        assert v["a"][0] >= DROP_BARS and v["b"][0] >= DROP_BARS, (model, cw, c, v)
        assert v["c"][0] >= SWAP_BARS, (model, cw, c, v)


BLIND_CELLS = (2100, 3000)


@pytest.mark.parametrize("model", ["vcond", "vcond_mf_hw0"])
@pytest.mark.parametrize("Nc", BLIND_CELLS)
def test_the_block_bar_does_not_see_one_cell_of_ordinary_counts(model, Nc):
    """The blind spot: `_problem`'s random Poisson counts, the U-only models, the faults planted as for 130 cells per wave, against
    the BLOCK-wise bar (2e-3 of the block's max-norm).  Held where the suite's U-only problems and every real data set live, from
    2 100 cells up: one cell is 1 / Nc of a row, so at the probe's own 402 .. 1 171 cells ordinary counts show a dropped cell at
    1.3 - 6.5 block bars (printed below, not asserted: the probe's shapes are small so that a gene is lit in few cells, not because
    ordinary counts would hide a cell there), at 2 100 cells at <= 1.5, at the benchmark's 50 000 far below."""
    p, par, eps = point_of(model, Nc, 70, False, lit=False)
    f = _faults(p, par, eps, planted_cells(130, Nc))
    high = {n: max(v[n][1] for v in f.values()) for n in "ab"}
    print(f"[cell rows] ordinary counts, {model} {Nc}x70: strongest planted fault, block bars: left out {high['a']:.2f}, twice {high['b']:.2f}")
    assert max(high.values()) < BLIND_BARS, (model, Nc, f)
    if Nc == BLIND_CELLS[0]:
        for cw in (1, 17, 130):
            n = probe_cells(cw)
            q, par, eps = point_of(model, n, 70, False, lit=False)
            g = _faults(q, par, eps, planted_cells(cw, n))
            print(f"[cell rows] ordinary counts, {model} {n}x70 (a probe shape): left out "
                  f"{min(v['a'][1] for v in g.values()):.2f} .. {max(v['a'][1] for v in g.values()):.2f} block bars")


def test_the_comparator_rejects_what_it_is_for():
    p = build("vcond_mf_hw0", probe_cells(65), 70)
    par, eps = point(p, False)
    _, g, _, _ = orc.loss_and_grads(p, par, eps)
    ratio = H.assert_gene_rows_match_oracle(g, par, p, eps, "float64 against itself")
    assert set(ratio) == {"ν_locs", "ν_scales", "logγg_locs", "logγg_scales", "logβg_locs", "logβg_scales", "shape_inv_locs"}
    assert all(v == 0.0 for v in ratio.values())
    wrong = orc.loss_and_grads(exchanged(p, 2 * 65 + 63), par, eps)[1]
    with pytest.raises(AssertionError):
        H.assert_gene_rows_match_oracle(wrong, par, p, eps, "a cell with its neighbour's counts")
    # per cell where phi_xy is learned, LRMN blocks by their gene rows
    q = build("vjoint_lrmn", probe_cells(17), 70)
    par, eps = point(q, True)
    _, g, _, _ = orc.loss_and_grads(q, par, eps)
    blocks = H.gene_row_blocks(g, q)
    assert blocks["ϕxy_locs"].shape == (698, 2) and blocks["cov_factor[γ]"].shape == (70, q.rho_rank) and blocks["loc[γ]"].shape == (70, 1)
    assert np.array_equal(blocks["loc[γ]"][:, 0], g["loc"].numpy()[:70]) and "rho_real_loc" in blocks
    bad = {k: v.clone() for k, v in g.items()}
    bad["ϕxy_locs"][40, 1] *= 1.01
    with pytest.raises(AssertionError):
        H.assert_gene_rows_match_oracle(bad, par, q, eps, "one cell's phi_xy row")
