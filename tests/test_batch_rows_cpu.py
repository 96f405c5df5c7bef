"""CPU: the power of the per-batch comparator (tests/helpers.py: assert_dnu_rows_match_oracle), on the float64 oracle alone.

The GPU suites hold d(-ELBO) / d Δν[q, g] of one-hot batches row by row at Δν = 0.  Here the "device" is the oracle itself with a
wrong batch design: a cell accounted to the neighbouring batch, one 8-cell chunk of a long batch accounted to the next batch, a
batch's row left out.  The comparator must reject each of them and accept the oracle's own float32 run with a wide margin (so that it
needs no float32-oracle clause) -- while the block-wise 3e-3 bar of tests/test_hip_sweep.py::_check, at parameters perturbed the way
`_check` perturbs them, accepts the misplaced cell: the gap the per-row bar closes."""
import numpy as np
import pytest
import torch

from oracle import velocycle_oracle as orc
from tests import helpers as H
from tests.test_hip_sweep import _problem

NC, NG, NB = 800, 70, 9
TINY, LONG = 4, 0          # onehot_layout("planted"): batch 4 has three cells, batch 0 has 400


def _planted(kind):
    if kind == "velocity":
        p = _problem("velocity", "meanfield", "NegativeBinomial", 1, 1, NB, 2, [], Nc=NC, Ng=NG, seed=901)
    else:
        p = _problem("phase", "meanfield", "NegativeBinomial", 2, 0, NB, 0, [], Nc=NC, Ng=NG, seed=902)
    ids = H.onehot_layout(NC, "planted", NB)
    p.Db = H.onehot_Db(ids, NB)
    return p, ids


def _perturbed(p):
    """Parameters and draws as tests/test_hip_sweep.py::_check forms them."""
    gen = torch.Generator().manual_seed(1)
    first = orc.draw_eps(p, gen)
    eps = orc.draw_eps(p, gen)
    par = orc.init_params(p, first.get("_cov_factor_draw"))
    for k in par:
        if torch.isfinite(par[k]).all():
            par[k] = par[k] + 0.05 * torch.randn(par[k].shape, generator=gen, dtype=torch.float64)
    return par, {k: v for k, v in eps.items() if not k.startswith("_")}


def _dnu_grad(p, ids, par, eps, dtype=torch.float64):
    q = orc.Problem(**{**p.__dict__, "Db": H.onehot_Db(ids, NB)}).to(dtype)
    _, g, _, _ = orc.loss_and_grads(q, {k: v.to(dtype) for k, v in par.items()}, {k: v.to(dtype) for k, v in eps.items()})
    return g["Δν_locs"].double().numpy()


def _mutations(ids):
    """{name: batch ids of the wrong design}: what a kernel that mis-assigns cells to batches computes."""
    tiny = torch.nonzero(ids == TINY).reshape(-1)
    assert tiny.numel() == 3 and int((ids == 2).sum()) == 0 and int((ids == LONG).sum()) == 400
    one_cell = ids.clone()
    one_cell[tiny[-1]] = TINY + 1                       # the last of the three cells counted with the batch behind it
    chunk = ids.clone()
    chunk[392:400] = LONG + 1                           # the last 8-cell chunk of batch 0 counted with batch 1
    return {"one cell of the 3-cell batch": one_cell, "one chunk of the 400-cell batch": chunk}


@pytest.fixture(scope="module", params=["velocity", "phase"])
def planted(request):
    p, ids = _planted(request.param)
    par, eps = _perturbed(p)
    par0 = dict(par, **{"Δν_locs": torch.zeros_like(par["Δν_locs"])})
    return dict(kind=request.param, p=p, ids=ids, par=par, par0=par0, eps=eps, want=_dnu_grad(p, ids, par0, eps))


def test_layouts_are_what_the_gpu_tests_rely_on():
    for Nb in (8, 9):
        ids = H.onehot_layout(NC, "planted", Nb)
        n = np.bincount(ids.numpy(), minlength=Nb)
        assert ids.numel() == NC and n[0] == 400 and n[7] == 264 and n[2] == 0 and n[4] == 3 and (np.diff(ids.numpy()) >= 0).all()
        rest = np.delete(n, [0, 7, 2, 4])
        assert rest.sum() == NC - 667 and rest.max() - rest.min() <= 1 and rest.min() > 3
    a = H.onehot_layout(NC, "interleaved", 7)
    b = H.onehot_layout(NC, "contiguous", 7)
    assert (np.diff(a.numpy()) < 0).any() and (np.diff(b.numpy()) >= 0).all()
    assert np.array_equal(np.bincount(a.numpy(), minlength=7), np.bincount(b.numpy(), minlength=7))
    given = torch.arange(NC) % 5
    assert torch.equal(H.onehot_layout(NC, "interleaved", 5, ids=given), given)
    assert torch.equal(H.onehot_layout(NC, "contiguous", 5, ids=given), torch.sort(given, stable=True).values)


def test_the_comparator_accepts_the_oracle_and_its_float32_run(planted):
    d = planted
    assert not bool(d["par0"]["Δν_locs"].any())
    assert H.assert_dnu_rows_match_oracle(d["want"], d["want"], "float64 against itself").max() == 0.0
    assert np.abs(d["want"][2]).max() == 0.0            # the empty batch: the row is the likelihood sum over no cells
    g32 = _dnu_grad(d["p"], d["ids"], d["par0"], d["eps"], torch.float32)
    ratio = H.assert_dnu_rows_match_oracle(g32, d["want"], "float32 oracle")
    print(f"[{d['kind']}] float32 oracle, worst err / bar per row: {np.array2string(ratio, precision=5)}")
    # a hundred times inside the bar: the comparator needs no "4 x the float32 oracle" clause
    assert ratio.max() <= 1e-2, ratio


def test_the_comparator_rejects_cells_in_the_wrong_batch(planted):
    d = planted
    for name, wrong in _mutations(d["ids"]).items():
        got = _dnu_grad(d["p"], wrong, d["par0"], d["eps"])
        with pytest.raises(AssertionError):
            H.assert_dnu_rows_match_oracle(got, d["want"], name)
        moved = np.abs(got - d["want"]).max(axis=1) / (H.DNU_ROW_RTOL * np.maximum(np.abs(d["want"]).max(axis=1), H.DNU_ROW_FLOOR))
        print(f"[{d['kind']}] {name}: err / bar per row {np.array2string(moved, precision=1)}")
        # BOTH rows involved are over the bar (the batch that lost the cells and the one that got them), no other row moves
        src, dst = (TINY, TINY + 1) if "3-cell" in name else (LONG, LONG + 1)
        assert moved[src] > 1.0 and moved[dst] > 1.0
        assert np.delete(moved, [src, dst]).max() == 0.0


def test_the_comparator_rejects_a_batch_left_out(planted):
    d = planted
    got = d["want"].copy()
    got[TINY] = 0.0
    with pytest.raises(AssertionError):
        H.assert_dnu_rows_match_oracle(got, d["want"], "the 3-cell batch's row zeroed")


def test_the_block_wise_bar_at_perturbed_offsets_accepts_the_misplaced_cell():
    """What tests/test_hip_sweep.py::_check asserts on the Δν_locs block (3e-3 of the BLOCK's max-norm, every parameter perturbed by
    0.05): with the velocity model's Normal(0, 0.01) prior the prior term, ~Δν / 1e-4, sets that max-norm, and the misplaced cell
    passes.  This is the gap; the test above shows the per-row bar at Δν = 0 closing it."""
    p, ids = _planted("velocity")
    par, eps = _perturbed(p)
    assert float(par["Δν_locs"].abs().max()) > 0.05
    want = _dnu_grad(p, ids, par, eps)
    got = _dnu_grad(p, _mutations(ids)["one cell of the 3-cell batch"], par, eps)
    err, bar = np.abs(got - want).max(), 3e-3 * max(np.abs(want).max(), 1e-2)
    print(f"block-wise bar {bar:.3f}, the misplaced cell moves the block by {err:.3f}")
    assert 0.0 < err <= bar
