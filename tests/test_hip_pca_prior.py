"""GPU: the two kernels of csrc/vc_pca.hip through the C ABI (vc_pca_stage, vc_pca_apply) against float64 numpy, and the PCA phase
prior end to end on the device (Phases.from_pca_heuristic(device="cuda")) against the float64 checker of tests/pca_checker.py.

vc_pca_apply is measured the way the project measures a float32 sum: Y in units of eps32 sum_g |xc||q|, Z in units of
eps32 sum_c |xc||y| (xc = X - mu in float64, X the device's own staged matrix, y the Y that the Z under test was formed from), and
the bar is 4 x the worst such ratio of a float32 torch-CPU matmul on the same inputs."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import pca_checker as PC

pytestmark = pytest.mark.gpu
FIX = range(len(PC.FIXTURES))
EPS32 = PC.EPS32
# (name, Nc, Ng, row stride, max_workgroups): the four fixtures; single, short and just-over-one tiles below 64 genes; more 64-cell
# tiles than workgroups on a padded row stride (Z's accumulators rest in the LDS between a workgroup's tiles); more than one gene
# group (2 048 genes) with a ragged last block, with one tile per workgroup and with two (the accumulators rest in the partial row)
SHAPES = [(f"fixture{i}", nc, ng, ng, 0) for i, (nc, ng, _) in enumerate(PC.FIXTURES)] + \
         [("one_cell", 1, 33, 33, 0), ("cells63", 63, 33, 33, 0), ("cells65", 65, 33, 33, 0), ("many_tiles", 33000, 16, 24, 0),
          ("two_groups", 130, 2100, 2104, 0), ("two_groups_two_tiles", 130, 2100, 2104, 2), ("fixture1_three_tiles", 1500, 97, 97, 8)]
SAME_MATRIX = {"two_groups_two_tiles": "two_groups", "fixture1_three_tiles": "fixture1"}


def _lib():
    from velocycle_amd import _lib as L
    return L, L.load()


def ptr(t):
    return C.c_void_p(t.data_ptr())


def raw_values(name, Nc, Ng):
    if name.startswith("fixture"):
        return PC.layer(int(name[-1]))
    if Ng == 33:
        return PC.layer(3)[:Nc]
    g = np.random.default_rng(Nc + Ng)
    return (g.gamma(0.7, 3.0, size=(Nc, Ng)) * (g.random((Nc, Ng)) < 0.6)).astype(np.float32)


def stage(v, stride, chunk=None, small=PC.SMALL):
    """vc_pca_stage over the whole of v in chunks: (X [Nc][stride] device, colsum float64 device, flag)"""
    L, lib = _lib()
    Nc, Ng = v.shape
    dev = torch.device("cuda:0")
    X = torch.full((Nc, stride), float("nan"), dtype=torch.float32, device=dev)
    colsum = torch.zeros(Ng, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    step = chunk or Nc
    for c0 in range(0, Nc, step):
        blk = torch.from_numpy(np.array(v[c0:c0 + step])).to(dev)
        n = blk.shape[0]
        partial = torch.empty(((n + 63) // 64, Ng), dtype=torch.float64, device=dev)
        rc = lib.vc_pca_stage(ptr(blk), n, Ng, Ng, C.c_float(small), ptr(X[c0]), stride, ptr(colsum), ptr(partial), ptr(flag), None)
        assert rc == L.VC_OK, lib.vc_last_error(None)
        torch.cuda.synchronize()
    return X, colsum, int(flag.item())


@lru_cache(maxsize=None)
def staged(name):
    _, Nc, Ng, stride, _ = next(s for s in SHAPES if s[0] == name)
    return stage(raw_values(name, Nc, Ng), stride)


def apply(X, Nc, Ng, stride, mu, Q, max_wg=0):
    L, lib = _lib()
    dev = X.device
    n_ws = int(lib.vc_pca_apply_workspace(Nc, Ng, max_wg))
    assert n_ws <= (max_wg or 512) * Ng * 8 and n_ws <= (Nc + 63) // 64 * Ng * 8
    ws = torch.full((n_ws,), float("nan"), dtype=torch.float32, device=dev)
    Y = torch.full((Nc, 8), float("nan"), dtype=torch.float32, device=dev)
    Z = torch.full((Ng, 8), float("nan"), dtype=torch.float64, device=dev)
    rc = lib.vc_pca_apply(ptr(X), Nc, Ng, stride, ptr(mu), ptr(Q), ptr(Y), ptr(Z), ptr(ws), n_ws, max_wg, None)
    assert rc == L.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    return Y.cpu(), Z.cpu()


@pytest.mark.parametrize("i", FIX)
def test_stage_logarithm_and_column_means(i):
    v = PC.layer(i)
    Nc, Ng = v.shape
    X, colsum, flag = staged(f"fixture{i}")
    assert flag == 0
    X = X.cpu().numpy()
    want = np.log(v.astype(np.float64) + PC.SMALL)
    err = np.abs(X - want) / np.maximum(1.0, np.abs(X))
    print(f"{PC.FIXTURES[i]}: staged logarithm off by {err.max() / EPS32:.3f} eps32 max(1, |X|)")
    assert err.max() <= 2 * EPS32
    mean = colsum.cpu().numpy() / Nc
    own = X.astype(np.float64).mean(0)
    rel = np.abs(mean - own).max() / np.abs(own).max()
    print(f"{PC.FIXTURES[i]}: column means off the float64 mean of the staged matrix by {rel:.2e} (relative)")
    assert np.abs(mean - own).max() <= 1e-12 * np.abs(own).max()


def test_stage_does_not_depend_on_the_chunks_and_latches_bad_values():
    v = PC.layer(2)                                                # 517 cells: 8 full tiles and one of 5
    X0, s0, _ = staged("fixture2")
    for chunk in (64, 192):
        X, s, flag = stage(v, v.shape[1], chunk)
        assert flag == 0 and torch.equal(X, X0) and torch.equal(s, s0), chunk
    for bad in (-PC.SMALL, -3.0, np.nan, np.inf):
        w = v.copy()
        w[300, 7] = bad
        assert stage(w, v.shape[1], 192)[2] == 1, bad
    L, lib = _lib()
    one = C.c_void_p(64)                                           # never dereferenced: refused before anything is launched
    assert lib.vc_pca_stage(one, 4, 16, 15, C.c_float(1.0), one, 16, one, one, one, None) == L.VC_ERR_ARG
    assert b"stride" in lib.vc_last_error(None)
    assert lib.vc_pca_stage(one, 4, 16, 16, C.c_float(1.0), one, 16, None, one, one, None) == L.VC_ERR_ARG
    assert lib.vc_pca_apply(one, 4, 16, 15, one, one, one, one, one, 1 << 20, 0, None) == L.VC_ERR_ARG
    assert lib.vc_pca_apply(one, 4, 16, 16, one, one, one, one, one, 8 * 16 - 1, 0, None) == L.VC_ERR_ARG
    assert b"workspace" in lib.vc_last_error(None)


@pytest.mark.parametrize("name,Nc,Ng,stride,max_wg", SHAPES, ids=[s[0] for s in SHAPES])
def test_apply_against_float64(name, Nc, Ng, stride, max_wg):
    Xd, colsum, flag = staged(SAME_MATRIX.get(name, name))
    assert flag == 0
    if Ng == 33:                                                   # the first cells of fixture 3 around ITS mean (one cell around its
        colsum, Nc_mu = staged("fixture3")[1], PC.FIXTURES[3][0]   # own mean would be a matrix of zeros)
    else:
        Nc_mu = Nc
    mu = (colsum.cpu() / Nc_mu).to(torch.float32)
    gen = torch.Generator().manual_seed(11)
    Q = torch.linalg.qr(torch.randn((Ng, 8), generator=gen, dtype=torch.float64))[0].to(torch.float32).contiguous()     # (LAPACK hands back column-major)
    Y, Z = apply(Xd, Nc, Ng, stride, mu.cuda(), Q.cuda(), max_wg)
    X = Xd.cpu()[:, :Ng]
    xc = X.double() - mu.double()
    unit_y = EPS32 * (xc.abs() @ Q.double().abs())
    # the float32 reference on the same inputs
    xc32 = X - mu
    Y32 = xc32 @ Q
    Z32 = xc32.T @ Y32
    def ratio(err, unit):                                          # an element whose terms are all zero must be exact
        assert bool((err[unit == 0] == 0).all())
        return float((err / unit.clamp_min(1e-300)).max())
    ry = lambda y: ratio((y.double() - xc @ Q.double()).abs(), unit_y)
    rz = lambda z, y: ratio((z.double() - xc.T @ y.double()).abs(), EPS32 * (xc.abs().T @ y.double().abs()))
    got_y, got_z, ref_y, ref_z = ry(Y), rz(Z, Y), ry(Y32), rz(Z32, Y32)
    print(f"{name} ({Nc} x {Ng}, stride {stride}): Y {got_y:.3f} (torch float32 {ref_y:.3f}), Z {got_z:.3f} (torch float32 {ref_z:.3f})"
          "  [eps32 sum |xc||q|, eps32 sum |xc||y|]")
    assert bool(torch.isfinite(Y).all()) and bool(torch.isfinite(Z).all())
    assert got_y <= 4 * ref_y, (got_y, ref_y)
    assert got_z <= 4 * ref_z, (got_z, ref_z)
    # bit-identical on repetition; the padding of the rows is not read
    Y2, Z2 = apply(Xd, Nc, Ng, stride, mu.cuda(), Q.cuda(), max_wg)
    assert torch.equal(Y, Y2) and torch.equal(Z, Z2)


@pytest.mark.parametrize("i", FIX)
def test_scores_against_the_oracle(i):
    PC.check_scores(i, "cuda")


@pytest.mark.parametrize("i", FIX)
def test_angles_against_the_oracle(i):
    PC.check_angles(i, "cuda")


@pytest.mark.parametrize("i", FIX)
def test_signs_are_sklearns(i):
    PC.check_signs(i, "cuda")


def test_zero_at_min_density_picks_the_oracles_cell():
    PC.check_min_density("cuda")


def test_variants_give_the_same_bits():
    PC.check_variants("cuda")


def test_refusals(monkeypatch):
    PC.check_refusals("cuda", monkeypatch)


@pytest.mark.parametrize("i", FIX)
def test_device_agrees_with_the_torch_loop(i):
    a, b = PC.prior(i, "cuda"), PC.prior(i, "cpu")
    err = float(np.abs(a.pcs - b.pcs).max())
    print(f"{PC.FIXTURES[i]}: normalised pcs cuda vs cpu {err:.3e}, bar {PC.bar(i):.3e}; iterations {a.pca.n_iter_} / {b.pca.n_iter_}")
    assert err <= PC.bar(i)
    assert abs(a.pca.n_iter_ - b.pca.n_iter_) <= 2
