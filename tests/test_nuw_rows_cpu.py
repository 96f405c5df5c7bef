"""CPU: the cases and the power of the per-condition comparator of the angular-speed coefficients (tests/helpers.py:
assert_nuw_rows_match_oracle), on the oracle alone.

d loglik / d nu_omega[x, h] = sum_c A3_c D[x, c] zeta_omega_h(phi_c) has one row per condition x.  tests/test_hip_nuw_paths.py holds
every such row of every step path to the float64 oracle within 2e-3 of the ROW's likelihood part.  This file owns the case table both
files run (CASES / build), asserts on every entry the conditions under which that bar means something -- the float32 oracle's own
rows within 0.25 of it (no float32-oracle clause needed: the device's error is 2.87 x the float32 oracle's at the 90 % quantile,
DESIGN section 4), every condition with cells carrying a likelihood part of at least 1 (the floor is not what passes it) -- and
keeps the argument as a regression: three planted mistakes of a per-condition sum are each at least 3 x over the row bar, while the
block-wide bar (2e-3 of the max-norm of the whole `νω_locs` / `loc` gradient) accepts the misplaced cell."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import velocycle_oracle as orc
from tests import helpers as H
from tests.test_hip_batch_paths import MODELS as _BATCH_MODELS, VCOND_SITES
from tests.test_hip_sweep import _problem

NB = 9                     # onehot_layout("planted", 9): batch 4 has three cells, batch 2 none, batch 0 400, batch 7 264
TINY_BATCH = 4
MODELS = {"vcond": _BATCH_MODELS["vcond"],                                                   # LRMN, the tutorials' velocity stage
          "vcond_mf": ("velocity", "meanfield", "NegativeBinomial", 1, 1, 2, VCOND_SITES),      # ... and its mean-field twin
          "vjoint_h1": _BATCH_MODELS["vjoint_h1"], "vjoint_lrmn": _BATCH_MODELS["vjoint_lrmn"]}

Case = namedtuple("Case", "model layout order Nx Hw Nc Ng")
Case.__str__ = lambda c: f"{c.model}-{c.layout}-{c.order[:5]}-Nx{c.Nx}-Hw{c.Hw}-{c.Nc}x{c.Ng}"

PWL_SHAPES = [(2, 1), (4, 0), (8, 0), (3, 0), (2, 0)]      # (Nx, Hw): rows of 4 and 8 floats, condition columns at offsets 0 .. 7


def _table():
    out = []
    C = lambda *a, Nc=800, Ng=70: out.append(Case(*a, Nc, Ng))
    # the tutorial flow's U-only kernel (per-lane partials, or its wave reduction)
    for order in ("contiguous", "interleaved"):
        for Nx, Hw in PWL_SHAPES:
            C("vcond", "tiny_last", order, Nx, Hw)
            if Nx >= 3:
                C("vcond", "empty_cond", order, Nx, Hw)
        for Nx, Hw in ((2, 1), (8, 0)):
            C("vcond_mf", "tiny_last", order, Nx, Hw)
        C("vcond_mf", "empty_cond", order, 3, 0)
    for Nx, Hw in PWL_SHAPES:
        C("vcond", "scattered", "contiguous", Nx, Hw)
    for Nx, Hw in ((2, 1), (3, 0)):
        C("vcond_mf", "scattered", "contiguous", Nx, Hw)
    C("vcond", "tiny_last", "contiguous", 2, 1, Ng=130)                       # a second gene block at four genes per lane
    # the S+U kernel's own partials
    for m in ("vjoint_h1", "vjoint_lrmn"):
        for layout in ("tiny_last", "scattered"):
            for Nx, Hw in ((2, 1), (4, 0)):
                C(m, layout, "contiguous", Nx, Hw)
    # the cell blocks' partials: 9 and 63 coefficients (more than K_main delivers itself)
    for m in ("vcond", "vjoint_h1", "vjoint_lrmn"):
        for Nx, Hw in ((3, 1), (9, 3)):
            C(m, "tiny_last", "contiguous", Nx, Hw)
        C(m, "scattered", "contiguous", 3, 1)
    C("vjoint_h1", "tiny_last", "interleaved", 3, 1)
    # the unfused kernels on three 1024-cell blocks, the last one ragged
    for m in ("vcond", "vjoint_h1"):
        for Nx in (2, 3, 9):
            C(m, "tiny_last", "contiguous", Nx, 1, Nc=2100)
        C(m, "scattered", "contiguous", 3, 1, Nc=2100)
    # more than 768 partial rows at one cell per wave
    C("vcond", "tiny_last", "contiguous", 8, 0, Nc=3200, Ng=40)
    C("vjoint_h1", "tiny_last", "contiguous", 2, 1, Nc=3200, Ng=10)
    # the run-time-sized kernel set by itself (Hw = 4)
    C("vjoint_h1", "tiny_last", "contiguous", 2, 4)
    C("vjoint_h1", "scattered", "contiguous", 2, 4)
    assert len(set(out)) == len(out)
    return out


CASES = _table()
# A seed per case, 9000 + its place in the table -- except where that draw violates a condition asserted below (then another seed,
# never another number): {case: seed}
SEEDS = {
    Case(model='vcond', layout='empty_cond', order='contiguous', Nx=4, Hw=0, Nc=800, Ng=70): 11002,
    Case(model='vcond', layout='tiny_last', order='contiguous', Nx=8, Hw=0, Nc=800, Ng=70): 13003,
    Case(model='vcond', layout='empty_cond', order='contiguous', Nx=8, Hw=0, Nc=800, Ng=70): 17004,
    Case(model='vcond_mf', layout='tiny_last', order='contiguous', Nx=8, Hw=0, Nc=800, Ng=70): 20009,
    Case(model='vcond_mf', layout='empty_cond', order='contiguous', Nx=3, Hw=0, Nc=800, Ng=70): 13010,
    Case(model='vcond', layout='tiny_last', order='interleaved', Nx=2, Hw=1, Nc=800, Ng=70): 10011,
    Case(model='vcond', layout='tiny_last', order='interleaved', Nx=4, Hw=0, Nc=800, Ng=70): 13012,
    Case(model='vcond', layout='empty_cond', order='interleaved', Nx=4, Hw=0, Nc=800, Ng=70): 10013,
    Case(model='vcond', layout='tiny_last', order='interleaved', Nx=8, Hw=0, Nc=800, Ng=70): 12014,
    Case(model='vcond', layout='empty_cond', order='interleaved', Nx=8, Hw=0, Nc=800, Ng=70): 12015,
    Case(model='vcond', layout='tiny_last', order='interleaved', Nx=2, Hw=0, Nc=800, Ng=70): 10018,
    Case(model='vcond_mf', layout='tiny_last', order='interleaved', Nx=8, Hw=0, Nc=800, Ng=70): 25020,
    Case(model='vcond', layout='scattered', order='contiguous', Nx=3, Hw=0, Nc=800, Ng=70): 10025,
    Case(model='vcond', layout='scattered', order='contiguous', Nx=2, Hw=0, Nc=800, Ng=70): 10026,
    Case(model='vcond_mf', layout='scattered', order='contiguous', Nx=2, Hw=1, Nc=800, Ng=70): 10027,
    Case(model='vcond_mf', layout='scattered', order='contiguous', Nx=3, Hw=0, Nc=800, Ng=70): 20028,
    Case(model='vcond', layout='tiny_last', order='contiguous', Nx=2, Hw=1, Nc=800, Ng=130): 11029,
    Case(model='vjoint_h1', layout='tiny_last', order='contiguous', Nx=4, Hw=0, Nc=800, Ng=70): 14031,
    Case(model='vjoint_h1', layout='scattered', order='contiguous', Nx=2, Hw=1, Nc=800, Ng=70): 10032,
    Case(model='vjoint_lrmn', layout='tiny_last', order='contiguous', Nx=4, Hw=0, Nc=800, Ng=70): 15035,
    Case(model='vcond', layout='tiny_last', order='contiguous', Nx=9, Hw=3, Nc=800, Ng=70): 13039,
    Case(model='vjoint_h1', layout='tiny_last', order='contiguous', Nx=9, Hw=3, Nc=800, Ng=70): 11042,
    Case(model='vjoint_h1', layout='scattered', order='contiguous', Nx=3, Hw=1, Nc=800, Ng=70): 10043,
    Case(model='vjoint_lrmn', layout='tiny_last', order='contiguous', Nx=3, Hw=1, Nc=800, Ng=70): 14044,
    Case(model='vjoint_lrmn', layout='tiny_last', order='contiguous', Nx=9, Hw=3, Nc=800, Ng=70): 10045,
    Case(model='vjoint_lrmn', layout='scattered', order='contiguous', Nx=3, Hw=1, Nc=800, Ng=70): 11046,
    Case(model='vcond', layout='tiny_last', order='contiguous', Nx=2, Hw=1, Nc=2100, Ng=70): 12048,
    Case(model='vjoint_h1', layout='tiny_last', order='contiguous', Nx=2, Hw=1, Nc=2100, Ng=70): 23052,
    Case(model='vjoint_h1', layout='tiny_last', order='contiguous', Nx=3, Hw=1, Nc=2100, Ng=70): 13053,
    Case(model='vjoint_h1', layout='scattered', order='contiguous', Nx=3, Hw=1, Nc=2100, Ng=70): 11055,
    Case(model='vjoint_h1', layout='tiny_last', order='contiguous', Nx=2, Hw=1, Nc=3200, Ng=10): 11057,
    Case(model='vjoint_h1', layout='scattered', order='contiguous', Nx=2, Hw=4, Nc=800, Ng=70): 11059,
}


def nuw_means(D):
    """Constant coefficients far apart: 0.2, 0.4, 0.6 for up to three conditions beside the tiny one (evenly over 0.2 .. 0.7 for
    more), 0.8 for the tiny (last) condition -- a cell evaluated with another condition's speed is an O(0.1) error, not a rounding.
    A condition WITHOUT cells gets 0.03, 0.06, ..: its row is the prior term (nu_omega - mu) / sd^2 alone, whose float32 rounding is
    ulp(nu_omega) / sd^2 -- at nu_omega = 0.6 and sd = 0.1 already 0.7 of the row's bar for the float32 oracle itself."""
    Nx = D.shape[0]
    step = 0.2 if Nx - 1 <= 3 else 0.5 / (Nx - 2)
    out = torch.tensor([0.2 + step * x for x in range(Nx - 1)] + [0.8], dtype=torch.float64)
    empty = torch.nonzero(D.sum(1) == 0).reshape(-1)
    out[empty] = 0.03 * (1 + torch.arange(empty.numel(), dtype=torch.float64))
    return out


@functools.lru_cache(maxsize=None)
def build(case):
    """The float64 oracle Problem of a case: data of tests.test_hip_sweep._problem, planted batches (in cell order, or shuffled:
    the engine then reorders the cells by batch), the condition design of helpers.condition_layout, nu_omega's prior means (= the
    guide's initial locations) of nuw_means."""
    kind, guide, noise, Hh, _, _, cond = MODELS[case.model]
    seed = SEEDS.get(case, 9000 + CASES.index(case) if case in CASES else 8999)
    p = _problem(kind, guide, noise, Hh, case.Hw, NB, case.Nx, cond, Nc=case.Nc, Ng=case.Ng, seed=seed)
    ids = H.onehot_layout(case.Nc, "planted", NB)
    if case.order == "interleaved":
        ids = ids[torch.randperm(case.Nc, generator=torch.Generator().manual_seed(seed))]
    p.Db = H.onehot_Db(ids, NB)
    p.D = H.condition_layout(ids, NB, case.Nx, case.layout)
    p.mu_nuw = p.mu_nuw.clone()
    p.mu_nuw[:, 0] = nuw_means(p.D)
    return p, ids


def point(p, perturbed, seed=1):
    """(parameters, draws), float32 values held in float64.  perturbed: init_params + 0.05 noise with Δν = 0, as
    tests/test_hip_sweep.py::_check forms them (what the unfused GPU cases evaluate); else the initial parameters themselves (where
    the first fused step evaluates, there with the device's own draws)."""
    gen = torch.Generator().manual_seed(seed)
    first = orc.draw_eps(p, gen)
    eps = orc.draw_eps(p, gen)
    par = orc.init_params(p, first.get("_cov_factor_draw"))
    if perturbed:
        for k in par:
            if torch.isfinite(par[k]).all():
                par[k] = par[k] + 0.05 * torch.randn(par[k].shape, generator=gen, dtype=torch.float64)
        if "Δν_locs" in par:
            par["Δν_locs"] = torch.zeros_like(par["Δν_locs"])
    return ({k: v.float().double() for k, v in par.items()},
            {k: v.float().double() for k, v in eps.items() if not k.startswith("_")})


def _loc_block(p):
    return "νω_locs" if p.guide == "meanfield" else "loc[νω]"


@functools.lru_cache(maxsize=None)
def _evaluate(case, perturbed):
    p, ids = build(case)
    par, eps = point(p, perturbed)
    want, lik, rest, bar = H.nuw_row_bars(par, p, eps)
    _, g32, _, _ = orc.loss_and_grads(p.to(torch.float32), {k: v.float() for k, v in par.items()}, {k: v.float() for k, v in eps.items()})
    got32 = H.nuw_row_blocks(g32, p)
    f32 = {k: H._rowmax(got32[k] - want[k]) / bar[k] for k in want}
    # per-cell contributions to the rows of the location block: d loss / d D[x(c), c] = d loss / d omega_c x omega_c
    leaves = {k: v.clone().requires_grad_(True) for k, v in par.items()}
    D = p.D.clone().requires_grad_(True)
    loss, _, det = orc.elbo_loss(orc.Problem(**{**p.__dict__, "D": D}), leaves, eps)
    loss.backward()
    cond = p.D.argmax(0)
    dw = D.grad.gather(0, cond[None])[0] / det["ω"].detach()
    G = (dw[:, None] * det["ζω"].detach().T).numpy()                                    # (Nc, Nhw)
    _, g64, _, _ = orc.loss_and_grads(p, par, eps)
    block = "νω_locs" if p.guide == "meanfield" else "loc"
    block_bar = 2e-3 * max(float(g64[block].abs().max()), 1e-3)
    return dict(p=p, ids=ids, cond=cond.numpy(), lik=lik, rest=rest, bar=bar, f32=f32, G=G, block_bar=block_bar)


def _mistakes(d):
    """{name: (condition, |change of that row of the location block| / row bar, the same / block bar)}."""
    p, G, cond, ids = d["p"], d["G"], d["cond"], d["ids"].numpy()
    bar = d["bar"][_loc_block(p)]
    tiny, Nx = p.Nx - 1, p.Nx
    n = np.bincount(cond, minlength=Nx)
    largest = int(n.argmax())
    a = np.abs(G[np.nonzero(ids == TINY_BATCH + 1)[0][0]]).max()
    b = np.abs(d["lik"][_loc_block(p)][tiny]).max()
    c = np.abs(G[np.nonzero(cond == largest)[0][-8:]].sum(0)).max()
    return {"a neighbouring batch's first cell added to the tiny row": (tiny, a / bar[tiny], a / d["block_bar"]),
            "the tiny row dropped to its prior part": (tiny, b / bar[tiny], b / d["block_bar"]),
            "the last 8-cell chunk of the largest condition left out": (largest, c / bar[largest], c / d["block_bar"])}


def test_layouts_are_what_the_gpu_tests_rely_on():
    ids = H.onehot_layout(800, "planted", NB)
    sizes = lambda D: D.sum(1).long().tolist()
    assert sizes(H.condition_layout(ids, NB, 3, "tiny_last")) == [452, 345, 3]
    assert sizes(H.condition_layout(ids, NB, 2, "tiny_last")) == [797, 3]
    assert sizes(H.condition_layout(ids, NB, 9, "tiny_last")) == [426, 27, 0, 27, 0, 27, 26, 264, 3]
    assert sizes(H.condition_layout(ids, NB, 3, "empty_cond")) == [797, 0, 3]
    assert sizes(H.condition_layout(ids, NB, 4, "empty_cond")) == [452, 0, 345, 3]
    with pytest.raises(ValueError):
        H.condition_layout(ids, NB, 2, "empty_cond")
    for name in ("tiny_last", "empty_cond"):
        for order in (ids, ids[torch.randperm(800, generator=torch.Generator().manual_seed(0))]):
            D = H.condition_layout(order, NB, 4, name)
            assert bool((D.sum(0) == 1).all()) and torch.equal(D[3].bool(), order == TINY_BATCH)
            for q in range(NB):                                    # constant within every batch
                assert len(set(D.argmax(0)[order == q].tolist())) <= 1
    D = H.condition_layout(ids, NB, 3, "scattered")
    assert bool((D.sum(0) == 1).all()) and torch.nonzero(D[2]).reshape(-1).tolist() == [0, 400, 799]
    assert len(set(D.argmax(0)[ids == 0].tolist())) > 1            # cuts through the batches
    assert nuw_means(H.condition_layout(ids, NB, 3, "tiny_last")).tolist() == pytest.approx([0.2, 0.4, 0.8])
    for Nx, name in ((9, "tiny_last"), (8, "empty_cond"), (3, "empty_cond")):
        m = nuw_means(H.condition_layout(ids, NB, Nx, name))
        assert float((m[:, None] - m[None, :]).abs().add(torch.eye(Nx)).min()) >= 0.029 and float(m[-1]) == 0.8


def test_row_blocks_of_both_guides():
    for model in ("vcond_mf", "vcond"):
        p, _ = build(Case(model, "tiny_last", "contiguous", 2, 1, 800, 70))
        par, eps = point(p, True)
        _, g, _, _ = orc.loss_and_grads(p, par, eps)
        blocks = H.nuw_row_blocks(g, p)
        if model == "vcond_mf":
            assert sorted(blocks) == ["νω_locs", "νω_scales"] and np.array_equal(blocks["νω_locs"], g["νω_locs"].numpy())
        else:
            assert sorted(blocks) == ["cov_diag[νω]", "cov_factor[νω]", "loc[νω]"]
            assert np.array_equal(blocks["loc[νω]"], g["loc"].numpy()[-6:].reshape(2, 3))
            assert blocks["cov_factor[νω]"].shape == (2, 3 * p.rho_rank)
            assert np.array_equal(blocks["cov_factor[νω]"][1, :p.rho_rank], g["cov_factor"].numpy()[-3])
        bad = {k: v.clone() for k, v in g.items()}
        bad["νω_locs" if model == "vcond_mf" else "loc"].reshape(-1)[-1] = float("inf")
        assert np.isnan(H.nuw_row_blocks(bad, p)[_loc_block(p)][1, 2])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_conditions_on_the_inputs_and_the_planted_mistakes(case):
    for perturbed in (True, False):
        d = _evaluate(case, perturbed)
        p = d["p"]
        cells = np.bincount(d["cond"], minlength=p.Nx)
        worst32 = max(float(v.max()) for v in d["f32"].values())
        low = float(H._rowmax(d["lik"][_loc_block(p)])[cells > 0].min())
        low_derived = min(float(H._rowmax(v)[cells > 0].min()) for v in d["lik"].values())
        print(f"[nuw rows] {case} {'perturbed' if perturbed else 'initial'}: float32 oracle / row bar {worst32:.3f}; smallest max|lik| of a "
              f"condition with cells {low:.2f} (location block), {low_derived:.3f} (all blocks)")
        # the conditions on the inputs.  max |lik[x]| >= 1 is held on the location block (`νω_locs`, `loc`): the rows d loglik /
        # d nu_omega themselves.  The scale-type blocks carry the same row times sd x draw (sd = 0.1: `νω_scales`, `cov_diag`) or
        # times a 0.02-sized factor entry x draw (`cov_factor`): there, ten times the floor -- the floor is not what passes a row
        assert worst32 <= 0.25, (case, perturbed, {k: np.round(v, 3) for k, v in d["f32"].items()})
        assert low >= 1.0, (case, perturbed, low)
        assert low_derived >= 10 * H.NUW_ROW_FLOOR, (case, perturbed, low_derived)
        # the D = 0 twin holds exactly the prior + entropy part: the rows of a condition without cells have no likelihood part
        for k, v in d["lik"].items():
            assert H._rowmax(v)[cells == 0].max(initial=0.0) <= 1e-9 * max(1.0, float(H._rowmax(d["rest"][k]).max())), (case, k)
        # the per-cell contributions are the rows
        loc = d["lik"][_loc_block(p)]
        sums = np.stack([d["G"][d["cond"] == x].sum(0) for x in range(p.Nx)])
        assert np.abs(sums - loc).max() <= 1e-9 * max(1.0, np.abs(loc).max()), (case, np.abs(sums - loc).max())
    # the hole, at the perturbed point (where the block-wide bars of tests/test_hip_sweep.py::_check are taken)
    m = _mistakes(_evaluate(case, True))
    print(f"[nuw rows] {case}: " + "; ".join(f"{k}: {r:.1f} x row bar, {b:.2f} x block bar" for k, (_, r, b) in m.items()))
    for k, (x, over_row, over_block) in m.items():
        assert over_row >= 3.0, (case, k, over_row)
    assert m["a neighbouring batch's first cell added to the tiny row"][2] <= 1.0, (case, m)


def test_the_block_bar_accepts_a_dropped_tiny_row_where_nothing_is_conditioned():
    hits = []
    for case in CASES:
        if case.model == "vjoint_h1":
            if _mistakes(_evaluate(case, True))["the tiny row dropped to its prior part"][2] <= 1.0:
                hits.append(str(case))
    print(f"the tiny condition's whole row is under the block bar on {len(hits)} evaluations: {hits}")
    assert hits


@pytest.mark.parametrize("model", ["vcond_mf", "vcond", "vjoint_h1", "vjoint_lrmn"])
def test_without_a_design_no_row_has_a_likelihood_part(model):
    """The `rest` of nuw_row_bars: with D = 0 (omega == 0) the nu_omega rows do not depend on the data at all."""
    p, _ = build(Case(model, "tiny_last", "contiguous", 3, 1, 800, 70))
    par, eps = point(p, True)
    p0 = orc.Problem(**{**p.__dict__, "D": torch.zeros_like(p.D)})
    other = orc.Problem(**{**p0.__dict__, "U": p.U.flip(1) + 3.0, "S": p.S if "ν" in p.condition_on else p.S.flip(1)})
    _, g0, _, _ = orc.loss_and_grads(p0, par, eps)
    _, g1, _, _ = orc.loss_and_grads(other, par, eps)
    a, b = H.nuw_row_blocks(g0, p), H.nuw_row_blocks(g1, p)
    for k in a:
        assert np.array_equal(np.nan_to_num(a[k]), np.nan_to_num(b[k])), k
    want, lik, rest, _ = H.nuw_row_bars(par, p0, eps)
    for k in lik:
        assert H._rowmax(lik[k]).max() == 0.0 and H._rowmax(rest[k]).max() > 0.0, k


def test_the_comparator_rejects_what_it_is_for():
    case = Case("vcond_mf", "tiny_last", "contiguous", 2, 1, 800, 70)
    assert case in CASES
    d = _evaluate(case, True)
    p = d["p"]
    par, eps = point(p, True)
    _, g, _, _ = orc.loss_and_grads(p, par, eps)
    ratio = H.assert_nuw_rows_match_oracle(g, par, p, eps, "float64 against itself")
    assert all(float(v.max()) == 0.0 for v in ratio.values())
    wrong = {k: v.clone() for k, v in g.items()}
    wrong["νω_locs"][1] += torch.tensor(d["G"][np.nonzero(d["ids"].numpy() == TINY_BATCH + 1)[0][0]])
    with pytest.raises(AssertionError):
        H.assert_nuw_rows_match_oracle(wrong, par, p, eps, "a neighbour's cell in the tiny row")
    H.assert_grads_match_oracle(orc.loss_and_grads(p, par, eps)[0], wrong, par, p, eps)        # ... which the block bars accept
