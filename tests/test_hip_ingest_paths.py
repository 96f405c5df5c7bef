"""GPU: every count-ingest path held to the dense answer -- CSR, strides, overflow.

Everything the likelihood kernels compute starts from the blocked count layout and the per-gene histograms that vc_finalize builds
(fin_pack_counts, csrc/vc_engine.hip), filled by vc_pack_counts_kernel (dense input, any strides, host or device memory) or by
vc_scatter_csr_kernel (CSR input: what AnnData layers hold).  A misplaced cell or gene there passes every oracle test, because the
oracle is handed the same dense matrix and not what the engine stored.  The bar between two ingest forms of one matrix is therefore
EQUALITY OF ENGINES (same_result): identical histograms, the same count storage / likelihood kernel / batch plan, the loss within
1e-13 (the per-gene lgamma constants are summed in another order: the bar of tests/test_hip_ingest.py) and every gradient bit for
bit on the same draws -- no measured tolerance: the two engines hold the same numbers in the same layout or they do not.  Each
family is anchored once to the float64 oracle at the bars of tests/helpers.py.

  a. CSR x one-hot batches that are not contiguous: only then the scatter kernel writes cell c to pos[c], while the dense kernel
     reads the inverse table (ord: position -> cell).  tests/test_ingest_cases_cpu.py shows that the two tables differ on every
     interleaved case and that scattering with the wrong one misplaces at least a quarter of the cells;
  b. the same on ranks 1 and 2 of 3;   c. Lognormal noise (log1p in the scatter kernel, no histogram), phase model without U;
  d. sparse structure (helpers.sparse_edge_counts);   e. values that change storage or histogram form, through CSR;
  f. dense strides: the three upload branches of vc_set_counts for host memory, and device sources with any strides;
  g. refusals on the CSR side;   h. the automatic host-histogram fallback past OVF_CAP = 2^22 overflow entries.
The case tables and builders below run on the host alone: tests/test_ingest_cases_cpu.py imports them."""
import copy
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from tests import helpers as H
from tests.helpers import _hist_equal, _host_checker, _mk
from tests.test_hip_batch_paths import _case, _first_step
from tests.test_hip_sweep import _problem

pytestmark = pytest.mark.gpu

OVF_CAP = 1 << 22                 # csrc/vc_engine.hip: overflow entries per matrix of the device histogram pass

BATCH_MODELS = ("phase_h2", "vjoint_h1", "vcond", "vjoint_poisson")
BATCH_LAYOUTS = (("interleaved", 3), ("interleaved", 9), ("contiguous", 7), ("planted", 9))
SHARD_LAYOUTS = (("interleaved", 9), ("planted", 9))


def batch_ng(layout, Nb):
    """Ng = 300 at four genes per lane (a second, ragged gene block of 44 genes) for one interleaved case per model."""
    return 300 if (layout, Nb) == ("interleaved", 9) else 70


def batch_cases():
    return [(m, layout, Nb, batch_ng(layout, Nb)) for m in BATCH_MODELS for layout, Nb in BATCH_LAYOUTS]


def batch_ids(spec):
    """The batch of every cell of a one-hot design (numpy int64, (Nc,))."""
    return spec.Db.argmax(0).numpy().astype(np.int64)


def batch_order(ids):
    """(ord, pos) of vc_order_by_batch (csrc/vc_host_logic.h): the cells stably sorted by batch -- ord[p] = the cell stored at
    position p of the blocked layout (what vc_pack_counts_kernel reads), pos[c] = the position of cell c (what
    vc_scatter_csr_kernel writes to)."""
    order = np.argsort(ids, kind="stable")
    pos = np.empty_like(order)
    pos[order] = np.arange(order.size)
    return order, pos


def to_csr(spec):
    """A shallow copy of `spec` that carries its counts as scipy CSR (cells x genes) only: HipEngine._setup -> vc_set_counts_csr."""
    out = copy.copy(spec)
    out.S_csr = sp.csr_matrix(spec.S.t().cpu().numpy())
    out.U_csr = sp.csr_matrix(spec.U.t().cpu().numpy()) if spec.U is not None else None
    out.S = out.U = None
    return out


def _draws(spec, seed=0):
    from velocycle_amd.rng import draw_eps
    g = torch.Generator().manual_seed(seed)
    first = draw_eps(spec, g)
    return first.get("_cov_factor_draw"), draw_eps(spec, g)


def _result(spec, draws, **kw):
    """Build an engine, evaluate one ELBO + gradient on `draws` from the initial parameters, close it: what same_result compares."""
    e = _mk(spec, **kw)
    try:
        e.init_params(draws[0])
        e.elbo_grad(eps=e.pack_eps(draws[1]))
        torch.cuda.synchronize()
        return dict(hist=e.histogram(), stats=dict(e.stats), loss=e.loss(), grad=torch.nan_to_num(e.grad[4:]).cpu(),
                    status=e.status())
    finally:
        e.close()


def same_result(a, b, hist=True):
    if hist:
        assert _hist_equal(a["hist"], b["hist"])
    for k in ("count_storage", "main_kernel", "onehot_batches"):
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    assert math.isfinite(b["loss"]) and abs(a["loss"] - b["loss"]) <= 1e-13 * abs(b["loss"]), (a["loss"], b["loss"])
    assert a["grad"].shape == b["grad"].shape and float(b["grad"].abs().max()) > 0.0
    assert torch.equal(a["grad"], b["grad"]), int((a["grad"] != b["grad"]).sum())


def same_engine(spec_a, spec_b, draws, hist=True, **kw):
    """The common assertion on two ingest forms of one problem; returns the two results."""
    a, b = _result(spec_a, draws, **kw), _result(spec_b, draws, **kw)
    same_result(a, b, hist)
    return a, b


# ---- a. CSR x batches ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,layout,Nb,Ng", batch_cases())
def test_csr_with_onehot_batches_equals_dense(model, layout, Nb, Ng):
    dense, tun = _case(model, layout, Nb, Ng)
    if layout == "interleaved":
        order, pos = batch_order(batch_ids(dense))
        assert not np.array_equal(order, pos)          # (a permutation that is its own inverse would hide a swap of the two tables)
    a, b = same_engine(dense, to_csr(dense), _draws(dense), tuning=tun)
    assert a["stats"]["onehot_batches"] == Nb == b["stats"]["onehot_batches"] and not b["stats"]["generic"]


@pytest.mark.parametrize("model", BATCH_MODELS)
def test_csr_with_interleaved_batches_against_the_oracle(model):
    """The anchor of group a: check 1 of tests/test_hip_batch_paths.py (the first fused step; assert_grads_match_oracle and
    assert_dnu_rows_match_oracle at their standing bars) on an engine that ingested CSR; the oracle sees the densified CSR."""
    dense, tun = _case(model, "interleaved", 3, 70)
    csr = to_csr(dense)
    assert csr.S is None and csr.U is None
    stats, ratio = _first_step(csr, tun, 3, f"CSR {model} interleaved Nb=3")
    assert stats["onehot_batches"] == 3
    if ratio is not None:
        print(f"[dnu rows, CSR ingest] {model}: worst err / bar {ratio:.2e}")


# ---- b. CSR x sharding --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("layout,Nb", SHARD_LAYOUTS)
@pytest.mark.parametrize("model", BATCH_MODELS)
def test_sharded_csr_with_batches_equals_dense(model, layout, Nb, rank):
    """Rank `rank` of 3: on the planted layout the rank lacks whole batches and its own cells are contiguous (pos == nullptr on that
    rank); on the interleaved one every rank reorders its own cells."""
    dense, tun = _case(model, layout, Nb, batch_ng(layout, Nb))
    draws = _draws(dense)
    a, b = same_engine(dense, to_csr(dense), draws, tuning=tun, rank=rank, world_size=3)
    whole = _mk(dense, tuning=tun)
    try:
        assert not _hist_equal(whole.histogram(), b["hist"])
    finally:
        whole.close()


# ---- c. CSR x noise and model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Nb", [0, 3])
@pytest.mark.parametrize("kind", ["phase", "velocity"])
def test_csr_lognormal_equals_dense(kind, Nb):
    """The log1p branch of the scatter kernel: float32 storage, no histogram; Nb = 3: interleaved batches (random ids)."""
    from velocycle_amd.tuning import Tuning
    Ng = 300 if Nb else 70
    p = _problem(kind, "meanfield", "Lognormal", 1, 1 if kind == "velocity" else 0, Nb, 2 if kind == "velocity" else 0, [],
                 Nc=661, Ng=Ng, seed=9100 + Nb + (10 if kind == "velocity" else 0))
    dense = H.spec_from_problem(p)
    if Nb:
        order, pos = batch_order(batch_ids(dense))
        assert not np.array_equal(order, pos)
    a, b = same_engine(dense, to_csr(dense), _draws(dense), hist=False, tuning=Tuning(genes_per_lane=4 if Ng > 70 else 0))
    for r in (a, b):
        assert r["hist"][1].size == 0 and r["hist"][2].size == 0 and not r["hist"][0].any()       # no histogram is built
        assert r["stats"]["count_storage"] == "f32" and r["stats"]["onehot_batches"] == Nb


def test_csr_lognormal_against_the_oracle():
    """The anchor of group c: one step of the CSR engine (velocity, Lognormal, interleaved batches) at assert_step_matches_oracle."""
    p = _problem("velocity", "meanfield", "Lognormal", 1, 1, 3, 2, [], Nc=661, Ng=70, seed=9113)
    csr = to_csr(H.spec_from_problem(p))
    draws = _draws(csr)
    e = _mk(csr)
    try:
        e.init_params(draws[0])
        e.elbo_grad(eps=e.pack_eps(draws[1]))
        H.assert_step_matches_oracle(e, csr, draws[1])
    finally:
        e.close()


def test_csr_phase_model_without_unspliced():
    """Phase model, negative binomial, no batches, no U_csr at all (`which = 1` never set); 300 genes at four per lane."""
    from velocycle_amd.tuning import Tuning
    from velocycle_amd.workloads import make_phase_spec
    dense = make_phase_spec(700, 300, seed=6)
    csr = to_csr(dense)
    assert csr.U_csr is None and csr.U is None and csr.S is None
    same_engine(dense, csr, _draws(dense), tuning=Tuning(genes_per_lane=4))
    same_engine(dense, csr, _draws(dense), tuning=Tuning(genes_per_lane=4), rank=1, world_size=3)


# ---- d. sparse structure ------------------------------------------------------------------------------------------------------------

SPARSE_NC, SPARSE_NG = 700, 300


@functools.lru_cache(maxsize=None)
def sparse_edge_specs(kind):
    """(dense spec, CSR spec as handed to the engine: explicit zeros, duplicates and unsorted rows still in it)."""
    from velocycle_amd.workloads import make_phase_spec, make_velocity_spec
    spec = make_phase_spec(SPARSE_NC, SPARSE_NG, seed=8) if kind == "phase" else \
        make_velocity_spec(SPARSE_NC, SPARSE_NG, "vjoint", 1, 1, seed=8)
    spec.truth = None
    mats = {"S": H.sparse_edge_counts(SPARSE_NC, SPARSE_NG, 31)}
    if kind != "phase":
        mats["U"] = H.sparse_edge_counts(SPARSE_NC, SPARSE_NG, 32)
    dense, csr = copy.copy(spec), copy.copy(spec)
    for k, (d, m) in mats.items():
        setattr(dense, k, torch.tensor(d).t().contiguous())
        setattr(csr, k, None)
        setattr(csr, k + "_csr", m)
    return dense, csr


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("kind", ["phase", "vjoint"])
def test_csr_sparse_structure_equals_dense(kind, world):
    from velocycle_amd.tuning import Tuning
    dense, csr = sparse_edge_specs(kind)
    raw = csr.S_csr
    assert not raw.has_canonical_format and int((raw.data == 0).sum()) >= 20        # handed over as built, not canonicalised
    kw = dict(tuning=Tuning(genes_per_lane=4))
    if world > 1:
        kw.update(rank=1, world_size=world)
    a, b = same_engine(dense, csr, _draws(dense), **kw)
    assert "u16" == b["stats"]["count_storage"]
    host = _host_checker(dense, **kw)
    try:
        assert _hist_equal(host.histogram(), b["hist"])
    finally:
        host.close()


# ---- e. values through CSR ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("overflow", list(H.OVERFLOW_VARIANTS), ids=lambda v: f"overflow_{v}")
@pytest.mark.parametrize("kind", ["phase", "vjoint"])
def test_csr_boundary_values_equal_dense(kind, overflow):
    dense = H.boundary_spec(kind, overflow=overflow)
    a, b = same_engine(dense, to_csr(dense), _draws(dense))
    assert b["stats"]["count_storage"] == H.OVERFLOW_VARIANTS[overflow][1] == a["stats"]["count_storage"]
    if overflow is not None:
        assert float(overflow) in b["hist"][1]


# ---- f. dense strides ---------------------------------------------------------------------------------------------------------------

STRIDE_NC, STRIDE_NG = 700, 300
STRIDE_FORMS = ("gene_major", "cell_major_T", "column_slice", "both_strided")


def strided_form(M, form):
    """The (Ng, Nc) float32 matrix M re-stored ON ITS DEVICE so that the returned view equals M with the strides of `form`.  The
    storage between the elements of the view holds -7: an element read from beside the view is refused as a negative count."""
    Ng, Nc = M.shape
    if form == "gene_major":                       # contiguous (Ng, Nc): gene_stride Nc, cell_stride 1
        return M.contiguous().clone()
    if form == "cell_major_T":                     # the reference's (Nc, Ng).T view: gene_stride 1, cell_stride Ng
        return M.t().contiguous().t()
    if form == "column_slice":                     # columns 20 .. 20 + Nc of a wider gene-major matrix: gene_stride Nc + 57 > Nc
        wide = torch.full((Ng, Nc + 57), -7.0, device=M.device)
        wide[:, 20:20 + Nc] = M
        return wide[:, 20:20 + Nc]
    if form == "both_strided":                     # big[::2, ::3]: gene_stride 6 Nc, cell_stride 3
        big = torch.full((2 * Ng, 3 * Nc), -7.0, device=M.device)
        big[::2, ::3] = M
        return big[::2, ::3]
    raise ValueError(form)


def stride_of(form, Ng=STRIDE_NG, Nc=STRIDE_NC):
    return {"gene_major": (Nc, 1), "cell_major_T": (1, Ng), "column_slice": (Nc + 57, 1), "both_strided": (6 * Nc, 3)}[form]


def upload_branch(gs, cs, Ng, Nc):
    """The host-memory branch of vc_set_counts (csrc/vc_engine.hip), restated: rows of Ng values at pitch cs; rows of Nc values at
    pitch gs -- tight (gs == Nc) or padded (gs > Nc: only this rank's columns of every row are uploaded); the whole span."""
    if gs == 1 and cs >= Ng:
        return "rows_of_genes"
    if cs == 1 and gs >= Nc:
        return "rows_of_cells_tight" if gs == Nc else "rows_of_cells_padded"
    return "whole_span"


@functools.lru_cache(maxsize=None)
def stride_base_spec():
    from velocycle_amd.workloads import make_velocity_spec
    spec = make_velocity_spec(STRIDE_NC, STRIDE_NG, "vjoint", 1, 1, seed=12)
    spec.truth = None
    return spec


def stride_spec(form, device="cpu"):
    base = stride_base_spec()
    spec = copy.copy(base)
    spec.S, spec.U = (strided_form(M.to(device), form) for M in (base.S, base.U))
    return spec


def test_dense_strides_host_and_device_give_one_engine():
    from velocycle_amd.tuning import Tuning
    base = stride_base_spec()
    draws = _draws(base)
    tun = Tuning(genes_per_lane=4)
    first = None
    for device in ("cpu", "cuda"):
        for form in STRIDE_FORMS:
            spec = stride_spec(form, device)
            # equal, positive strides on S and U: _setup hands the views over as they are
            assert spec.S.stride() == spec.U.stride() == stride_of(form), (form, spec.S.stride(), spec.U.stride())
            assert spec.S.is_cuda == (device == "cuda") and torch.equal(spec.S.cpu(), base.S) and torch.equal(spec.U.cpu(), base.U)
            r = _result(spec, draws, tuning=tun)
            if first is None:
                first = r
            else:
                same_result(r, first)
    # sharded: rank 1 of 3 of every host form (the row-wise uploads take this rank's cells only) against the contiguous device form
    ref = _result(stride_spec("gene_major", "cuda"), draws, tuning=tun, rank=1, world_size=3)
    assert not _hist_equal(ref["hist"], first["hist"])
    for form in STRIDE_FORMS:
        same_result(_result(stride_spec(form, "cpu"), draws, tuning=tun, rank=1, world_size=3), ref)


# ---- g. refusals --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _refusal_base():
    from velocycle_amd.workloads import make_velocity_spec
    spec = make_velocity_spec(600, 70, "vjoint", 1, 1, seed=15)
    spec.truth = None
    return spec


@pytest.mark.parametrize("which", ["S_csr", "U_csr"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -1.0])
def test_invalid_csr_values_are_refused(bad, which):
    csr = to_csr(_refusal_base())
    m = getattr(csr, which).copy()
    assert m.nnz > 1000
    m.data[m.nnz // 2] = bad
    setattr(csr, which, m)
    with pytest.raises(ValueError, match="finite and >= 0"):
        _mk(csr)


def test_set_counts_csr_after_finalize_is_refused():
    from velocycle_amd import _lib
    import ctypes as C
    csr = to_csr(_refusal_base())
    e = _mk(csr)
    try:
        m = csr.S_csr
        indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(m.indices, dtype=np.int32)
        data = np.ascontiguousarray(m.data, dtype=np.float32)
        assert indptr[0] == 0 and indptr[-1] == m.nnz and indptr.size == csr.Nc + 1          # valid host arrays
        rc = e.lib.vc_set_counts_csr(e._h, 0, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p),
                                     data.ctypes.data_as(C.c_void_p), int(m.nnz), 0)
        assert rc == _lib.VC_ERR_STATE
        assert b"after vc_finalize" in e.lib.vc_last_error(e._h)
    finally:
        e.close()


# ---- h. the overflow cap ------------------------------------------------------------------------------------------------------------

CAP_NG, CAP_NC_OVER, CAP_NC_UNDER = 2000, 2100, 2090


@functools.lru_cache(maxsize=None)
def cap_spec(Nc):
    """Phase model, negative binomial, Nc x 2000, every entry non-integer (counts + 0.25): Nc x 2000 overflow entries."""
    from velocycle_amd.workloads import make_phase_spec
    spec = make_phase_spec(Nc, CAP_NG, seed=21)
    spec.truth = None
    spec.S = spec.S.contiguous() + 0.25
    return spec


def _on_device(spec):
    out = copy.copy(spec)
    out.S = spec.S.cuda()
    return out


def test_overflow_cap_falls_back_to_the_host_pass():
    spec = cap_spec(CAP_NC_OVER)
    assert spec.S.numel() > OVF_CAP and bool((spec.S != spec.S.floor()).all())
    draws = _draws(spec)
    dev_spec = _on_device(spec)
    e = _mk(dev_spec)
    try:
        assert not e.stats["hist_on_device"] and e.stats["count_storage"] == "f32", e.stats
        host = _host_checker(dev_spec)
        try:
            assert _hist_equal(e.histogram(), host.histogram())
        finally:
            host.close()
        e.init_params(draws[0])
        e.elbo_grad(eps=e.pack_eps(draws[1]))
        H.assert_step_matches_oracle(e, spec, draws[1])
    finally:
        e.close()
    # host memory: the same engine
    a, b = same_engine(spec, dev_spec, draws)
    assert not a["stats"]["hist_on_device"] and not b["stats"]["hist_on_device"]


def test_overflow_cap_refuses_csr():
    csr = to_csr(cap_spec(CAP_NC_OVER))
    assert csr.S_csr.nnz > OVF_CAP
    with pytest.raises(NotImplementedError, match="CSR input with more than"):
        _mk(csr)


def test_below_the_overflow_cap_the_device_histograms_stay():
    spec = cap_spec(CAP_NC_UNDER)
    assert spec.S.numel() < OVF_CAP and bool((spec.S != spec.S.floor()).all())
    dev_spec = _on_device(spec)
    e, host = _mk(dev_spec), _host_checker(dev_spec)
    try:
        assert e.stats["hist_on_device"] and e.stats["count_storage"] == "f32", e.stats
        assert _hist_equal(e.histogram(), host.histogram())
    finally:
        e.close(); host.close()
