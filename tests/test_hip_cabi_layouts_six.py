"""GPU: the six later engine-less entry points of include/velocycle_hip.h -- vc_gene_glm_weighted, vc_gene_glm_batch_weighted,
vc_gene_kinetics_weighted, vc_cell_speed, vc_gene_joint, vc_gene_joint_weighted -- called directly in every layout their header allows
(tests/cabi_layouts.py; what the layouts are is checked without a device in tests/test_cabi_layouts_cpu.py).  The first five entry
points are held the same way in tests/test_hip_cabi_layouts.py.

Anchors: the `compact` direct call (the workers' convention) is packaged by the worker's own packaging where there is one, held to the
float64 checker at the standing bars of that kernel's own GPU test file -- through that file's `assert_within_bars` (vc_cell_speed,
vc_gene_joint), or as that file judges non-integer weights: the written-out float64 reference of the weighted formulas on the same
yardsticks and bars (the four weighted kernels; every case here has a weight that is no integer) -- and equals the Python worker bit
for bit on every output the worker hands through.  With a table of ones, R = 1 and strides 0 each weighted kernel equals its
unweighted sibling's compact call byte for byte.  Every other layout must then equal `compact` on every output, byte for byte, with
both guard bands of every output intact and everything outside a range untouched.  No tolerance of its own anywhere in this file."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cabi_layouts as L
from tests import cell_speed_checker as CS
from tests import gene_batch_boot_checker as BW
from tests import gene_batch_checker as BC
from tests import gene_boot_checker as W
from tests import gene_glm_checker as G
from tests import gene_joint_boot_checker as X
from tests import gene_joint_checker as J
from tests import gene_kinetics_boot_checker as KB
from tests import gene_kinetics_checker as Q
from tests import test_hip_cell_speed as TCS
from tests import test_hip_gene_batch_bootstrap as TBB
from tests import test_hip_gene_bootstrap as TGB
from tests import test_hip_gene_joint as TJ
from tests import test_hip_gene_joint_bootstrap as TJB
from tests import test_hip_gene_kinetics_bootstrap as TKB
from tests.test_hip_cabi_layouts import big, bits, unpacked                        # noqa: F401  (big: the module's 8.6 GB fixture)
from velocycle_amd import cell_speed as CSP
from velocycle_amd import gene_harmonics as GH
from velocycle_amd import gene_joint as GJ
from velocycle_amd import gene_kinetics as GK

pytestmark = pytest.mark.gpu

# a case is "<name of the checker's problem>[:nw0][:nocov]": nw0: NW = 0 (no design, no profile outputs); nocov: cov_dev (and the batch
# kernel's variance pair) NULL
CASES = {
    "glmw": ["shape_65_7_3_NegativeBinomial", "shape_257_5_1_Poisson", "shape_257_5_1_Poisson:nocov"],
    "batchw": ["seven_2_NegativeBinomial", "silent_batch", "silent_batch:nocov"],
    "kinw": ["score_257_5_3", "score_257_5_2:nocov", "shape_65_4_2_Poisson", "shape_257_5_1_NegativeBinomial:nw0"],
    "cell": ["shape_257_3_1_Poisson", "shape_64_65_2_NegativeBinomial", "shape_63_4_2_Poisson"],
    "joint": ["score_257_5_3", "score_257_5_2", "shape_65_4_2_Poisson", "shape_257_5_1_NegativeBinomial:nw0"],
    "jointw": ["score_257_5_3", "score_257_5_2:nocov", "shape_65_4_2_Poisson", "shape_257_5_1_NegativeBinomial:nw0"],
}
ANCHORS = {k: [c for c in v if ":" not in c] for k, v in CASES.items()}
WEIGHTED = ("glmw", "batchw", "kinw", "jointw")
ROW_TABLES = ("kinw", "jointw")
STORAGES = ("u16", "f32")
ALL = [(k, c, s) for k in CASES for c in CASES[k] for s in STORAGES]
LAYOUTS = [L.padded(1), L.padded(3), L.padded(61), L.window(5, 7), L.offset_inputs, L.side_stream]
WEIGHT_LAYOUTS = [L.weights_padded(1), L.weights_padded(61), L.row_range(1, 3), L.row_range(1, 2), L.both(L.padded(1), L.weights_padded(61)),
                  L.both(L.row_range(1, 3), L.weights_padded(1))]
ROW_LAYOUTS = [L.row_strides(1), L.row_strides(7), L.both(L.row_strides(7), L.weights_padded(61)), L.both(L.row_range(1, 3), L.row_strides(1)),
               L.both(L.row_range(2, 3), L.row_strides(7))]
CELL_RANGES = {257: [(3, 200), (65, 66), (130, 257)], 64: [(1, 63), (37, 38)], 63: [(1, 62), (5, 6)]}
BIG_CASES = {"glmw": "shape_257_5_1_NegativeBinomial", "batchw": "one_batch", "kinw": "shape_257_5_1_NegativeBinomial",
             "cell": "shape_257_3_1_Poisson", "joint": "shape_257_5_1_NegativeBinomial", "jointw": "shape_257_5_1_NegativeBinomial"}
ROWS = 3


def ids(params):
    return ["-".join(p) for p in params]


def names(layouts):
    return [lay.name for lay in layouts]


def weights(kernel, name):
    """float64 [3][Nc]: the first rows of the kernel's bootstrap checker's table, with a non-integer weight planted (`L.case_weights`)."""
    if kernel == "glmw":
        return L.case_weights(W.cases()[name][1], ROWS)
    if kernel == "batchw":
        return L.case_weights(BW.cases()[name][1], ROWS)
    return L.case_weights(KB.weights(name, ROWS) if kernel == "kinw" else X.weights(name, rows=ROWS), ROWS)


def problem(kernel, name):
    return {"glmw": lambda: W.cases()[name][0], "batchw": lambda: BW.cases()[name][0], "kinw": lambda: Q.cases()[name],
            "cell": lambda: CS.cases()[name], "joint": lambda: J.cases()[name], "jointw": lambda: J.cases()[name]}[kernel]()


@lru_cache(maxsize=None)
def spec(kernel, case, storage, form="layout", Wt=None):
    """form "layout": what the layout tests run -- warm starts, per-row tables ("rows"), a start and a prior per cell, so that every
    optional input is there and differs from row to row, gene to gene and cell to cell; "copies": the per-row tables R copies of row 0's;
    "plain": the workers' convention (shared tables, no start, no prior), what the anchors run.  Wt: another weight table, as a tuple of
    rows (row isolation, ones)."""
    name, *flags = case.split(":")
    cov, nw0 = "nocov" not in flags, "nw0" in flags
    p = problem(kernel, name)
    lay = form != "plain"
    tables = {"layout": "rows", "copies": "copies", "plain": "shared"}[form]
    w = np.array(Wt, dtype=np.float64) if Wt is not None else (weights(kernel, name) if kernel in WEIGHTED else None)
    if kernel == "glmw":
        return L.glm_weighted_spec(p, w, storage, warm=lay, want_cov=cov)
    if kernel == "batchw":
        return L.batch_weighted_spec(p, w, storage, warm=lay, want_var=cov)
    if kernel == "kinw":
        return L.kinetics_weighted_spec(p, w, storage, tables=tables, want_cov=cov, nw0=nw0)
    if kernel == "cell":
        return L.cell_speed_spec(p, storage, varied=lay)
    if kernel == "joint":
        return L.joint_spec(p, storage, nw0=nw0, start=lay)
    return L.joint_weighted_spec(p, w, storage, tables=tables, want_cov=cov, nw0=nw0)


@lru_cache(maxsize=None)
def compact(kernel, case, storage, form="layout"):
    s = spec(kernel, case, storage, form)
    out = L.direct_call(s, L.compact)
    assert out["guards_intact"] and out["outside_untouched"] and out["gene_stride"] == s["M"].shape[1]
    if kernel in WEIGHTED:
        assert out["weight_stride"] == s["M"].shape[1]
    return out


def outputs(res):
    return {k: v for k, v in res.items() if k not in L.OUTPUT_FLAGS}


def as_tuple(w):
    return tuple(tuple(float(x) for x in row) for row in np.asarray(w))


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def on_device(out, keys):
    return {k: torch.from_numpy(np.ascontiguousarray(out[k])).to(dev()) for k in keys}


def constants(blk32, r32, w64=None):
    """The workers' own lgamma constants of a spec's float32 block, on the device (w64: under one row of weights)."""
    r64 = r32.to(dev()).double() if r32 is not None else None
    return GH._constants(blk32.to(dev()), r64, torch.from_numpy(np.ascontiguousarray(w64)).to(dev()) if w64 is not None else None)


def same_fields(a, b, fields):
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f


# ------------------------------------------------------------------------------------------------- anchors: the unweighted kernels
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["cell"])
def test_anchor_cell_speed(case, storage):
    s, out = spec("cell", case, storage, "plain"), compact("cell", case, storage, "plain")
    at_start = L.direct_call(L.cell_speed_spec(CS.cases()[case], storage, max_iter=0), L.compact)
    assert at_start["guards_intact"] and (at_start["st"] == CS.EVALUATED).all()
    keys = ("omega", "var", "sums", "dec", "it", "st", "nc")
    r64 = s["r32"].to(dev()).double() if s["r32"] is not None else None
    shell = SimpleNamespace(const=CSP._cell_constants(s["blk32"].to(dev()), r64))
    fit = CSP._Problem.fit(shell, on_device(out, keys), None, CSP._score_z(at_start["sums"]))   # the worker's own packaging of the outputs
    TCS.assert_within_bars(case, fit)
    same_fields(fit, TCS.run(case), [f for f in CSP.CellSpeedFit.__dataclass_fields__])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["joint"])
def test_anchor_gene_joint(case, storage):
    s, out = spec("joint", case, storage, "plain"), compact("joint", case, storage, "plain")
    keys = ("theta", "cov", "lls", "llu", "dec", "it", "st", "nc", "score", "info")
    shell = SimpleNamespace(K=s["K"], D=s["K"] + 2, const_S=constants(s["blk32"], s["r32"]), const_U=constants(s["blk32_2"], s["r32"]))
    fit = GJ._Problem.fit(shell, on_device(out, keys))                                  # the worker's own packaging of the outputs
    assert fit.score_w.shape[1] == s["NW"] == J.cases()[case]["W"].shape[0]
    TJ.assert_within_bars(case, fit)
    same_fields(fit, TJ.run(case, storage=storage), [f for f in GJ.GeneJointFit.__dataclass_fields__])


# --------------------------------------------------------------------------------------------------- anchors: the weighted kernels
@lru_cache(maxsize=None)
def ones_call(kernel, case, storage):
    Nc = problem(kernel, case)["U" if kernel in ROW_TABLES else "S"].shape[0]
    out = L.direct_call(spec(kernel, case, storage, "plain", as_tuple(np.ones((1, Nc)))), L.compact)
    assert out["guards_intact"] and out["outside_untouched"] and out["row_strides"] in ((), (0, 0), (0, 0, 0))
    return out


def sibling(kernel, case, storage):
    p = problem(kernel, case)
    s = {"glmw": lambda: L.glm_spec(p, storage), "batchw": lambda: L.batch_spec(p, storage), "kinw": lambda: L.kinetics_spec(p, storage),
         "jointw": lambda: L.joint_spec(p, storage)}[kernel]()
    out = L.direct_call(s, L.compact)
    assert out["guards_intact"]
    return out


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kernel,case", [(k, c) for k in WEIGHTED for c in ANCHORS[k]], ids=lambda v: v)
def test_a_table_of_ones_is_the_unweighted_sibling(kernel, case, storage):
    """R = 1, a table of ones, all strides 0, no start: every output of the unweighted entry point, byte for byte."""
    got, want = outputs(ones_call(kernel, case, storage)), outputs(sibling(kernel, case, storage))
    L.assert_same_outputs({k: v[0] for k, v in got.items()}, want)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["glmw"])
def test_anchor_gene_glm_weighted(case, storage):
    p, Wt = problem("glmw", case), weights("glmw", case)
    s, out = spec("glmw", case, storage, "plain"), compact("glmw", case, storage, "plain")
    w32 = L.weights_of(s).astype(np.float64)
    bars, worst, judged = W.bars(), dict(coef=0.0, std=0.0), 0
    for b in range(ROWS):
        worker = TGB.run(p, cell_weights=Wt[b])                                        # the worker's one-row call is a row of this call
        cov = unpacked(out["cov"][b], s["K"])
        assert bits(out["nu"][b].T.copy(), worker.means) and bits(cov, worker.cov) and bits(out["dec"][b], worker.decrement)
        assert bits(out["it"][b], worker.iterations) and bits(out["st"][b], worker.status)
        assert bits(out["ll"][b] + constants(s["blk32"], s["r32"], w32[b]).cpu().numpy(), worker.loglik)
        for g in range(out["st"].shape[1]):
            k, B, logm, r, prior = G._gene_inputs(p, g)
            f64 = W.weighted_newton64(k, B, logm, w32[b], p["noisemodel"], r, prior)
            if f64["status"] != G.CONVERGED:
                continue
            judged += 1
            assert out["st"][b, g] in TGB.DONE, (case, b, g, out["st"][b, g])
            d = out["nu"][b, g] - f64["nu"]
            worst["coef"] = max(worst["coef"], float(np.sqrt(max(d @ f64["hess"] @ d, 0.0))))
            worst["std"] = max(worst["std"], float(np.abs(np.sqrt(np.diag(cov[g])) / f64["std"] - 1).max()))
    print(f"{case}: {judged} pairs; worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    assert judged >= ROWS * out["st"].shape[1] - 2 and all(worst[k] <= bars[k] for k in worst)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["batchw"])
def test_anchor_gene_glm_batch_weighted(case, storage):
    p, Wt = problem("batchw", case), weights("batchw", case)
    s, out = spec("batchw", case, storage, "plain"), compact("batchw", case, storage, "plain")
    w32 = np.ascontiguousarray(L._table32(Wt, Wt.shape[1]), dtype=np.float64)          # in the caller's cell order, like the checker's inputs
    bars, worst, judged = BW.bars(), dict(coef=0.0, std=0.0, dstd=0.0), 0
    for b in range(ROWS):
        worker = TBB.run(p, cell_weights=Wt[b])
        cov = unpacked(out["cov"][b], s["K"])
        assert bits(out["nu"][b].T.copy(), worker.means) and bits(out["delta"][b].T.copy(), worker.delta_nu) and bits(cov, worker.cov)
        assert bits(out["dec"][b], worker.decrement) and bits(out["it"][b], worker.iterations) and bits(out["st"][b], worker.status)
        for g in range(out["st"].shape[1]):
            f64 = BW.written_out64(*BC.gene_inputs(p, g)[:4], w32[b], p["noisemodel"], *BC.gene_inputs(p, g)[4:])
            if f64["status"] != G.CONVERGED:
                continue
            judged += 1
            assert out["st"][b, g] in TBB.DONE, (case, b, g, out["st"][b, g])
            K = s["K"]
            d = np.concatenate([out["nu"][b, g], out["delta"][b, g]]) - f64["nu"]
            worst["coef"] = max(worst["coef"], float(np.sqrt(max(d @ f64["hess"] @ d, 0.0))))
            worst["std"] = max(worst["std"], float(np.abs(np.sqrt(np.diag(cov[g])) / f64["std"][:K] - 1).max()))
            worst["dstd"] = max(worst["dstd"], float(np.abs(np.sqrt(out["dvar"][b, g]) / f64["std"][K:] - 1).max()))
    print(f"{case}: {judged} pairs; worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    assert judged >= ROWS * out["st"].shape[1] - 2 and all(worst[k] <= bars[k] for k in worst)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["kinw"])
def test_anchor_gene_kinetics_weighted(case, storage):
    p, Wt = problem("kinw", case), weights("kinw", case)
    s, out = spec("kinw", case, storage, "plain"), compact("kinw", case, storage, "plain")
    w32 = L.weights_of(s).astype(np.float64)
    keys = ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")
    r64 = s["r32"].to(dev()).double() if s["r32"] is not None else None
    shell = SimpleNamespace(const=GK._row_constants(s["blk32"].to(dev()), r64, torch.from_numpy(w32).to(dev())))
    shell.fit = lambda o, const=None: GK._Problem.fit(shell, o, const)
    fit = GK._Problem.fit_rows(shell, on_device(out, keys))                             # the worker's own packaging of the outputs
    same_fields(fit, TKB.fit_rows(p, Wt, storage=storage), [f for f in GK.GeneKineticsFit.__dataclass_fields__])
    bars, worst, judged = KB.bars(), dict(xy=0.0, cov=0.0, loglik=0.0), 0
    for b in range(ROWS):
        for g in range(out["st"].shape[1]):
            if not KB.has_data(p, w32[b], g):
                assert TKB.is_no_data(out, b, g), (case, b, g)
                continue
            k, B, logm, nu, r = Q.gene_inputs(p, g)
            f64 = KB.weighted_solve64(k, B, logm, nu, p["W"], p["nuw"], w32[b], p["noisemodel"], r)
            if f64["status"] != Q.CONVERGED or f64["minz"] < Q.MIN_Z:                   # the checker's tolerance-bearing pairs: kink-free
                continue
            judged += 1
            assert out["st"][b, g] in Q.INTERIOR and out["nc"][b, g] == 0, (case, b, g, out["st"][b, g])
            worst["xy"] = max(worst["xy"], Q.xy_distance(out["xy"][b, g, 0], out["xy"][b, g, 1], f64))
            worst["cov"] = max(worst["cov"], Q.sym_distance(TKB.cov2(out["cov"][b, g]), f64["inv"]))
            worst["loglik"] = max(worst["loglik"], Q.loglik_distance(out["ll"][b, g] + TKB.host_const(p, w32[b], g), f64))
    print(f"{case}: {judged} pairs; worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    assert judged >= ROWS * out["st"].shape[1] - 2 and all(worst[k] <= bars[k] for k in worst)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", ANCHORS["jointw"])
def test_anchor_gene_joint_weighted(case, storage):
    """From the bootstrap's warm start, as tests/test_hip_gene_joint_bootstrap.py judges non-integer weights (from the default start the
    first full step of some of these cases runs into the kink)."""
    p, Wt = problem("jointw", case), weights("jointw", case)
    starts = np.array(X.warm_starts(case))
    s = L.joint_weighted_spec(p, Wt, storage, start=starts)
    out = L.direct_call(s, L.compact)
    assert out["guards_intact"] and out["outside_untouched"] and out["row_strides"] == (0, 0)
    w32 = L.weights_of(s).astype(np.float64)
    keys = ("theta", "cov", "lls", "llu", "dec", "it", "st", "nc", "score", "info")
    worker = TJB.run_w(case, Wt, start=TJ.start_of(starts), storage=storage)
    D = s["K"] + 2
    r64, W64 = s["r32"].to(dev()).double() if s["r32"] is not None else None, torch.from_numpy(w32).to(dev())
    const_S, const_U = (GK._row_constants(s[k].to(dev()), r64, W64) for k in ("blk32", "blk32_2"))      # as the weighted worker forms them
    for b in range(ROWS):
        shell = SimpleNamespace(K=s["K"], D=D, const_S=const_S[b], const_U=const_U[b])
        fit = GJ._Problem.fit(shell, on_device({k: out[k][b] for k in keys}, keys))     # the worker's packaging, row by row
        same_fields(fit, TJB.row_of(worker, b), [f for f in GJ.GeneJointFit.__dataclass_fields__])
    bars, worst, judged = X.bars(), dict(theta=0.0, cov=0.0), 0
    for b in range(ROWS):
        for g in range(out["st"].shape[1]):
            if not X.has_data(p, w32[b], g):
                assert out["st"][b, g] == J.NO_DATA and np.isnan(out["theta"][b, g]).all(), (case, b, g)
                continue
            kS, kU, B, logm, r = J.gene_inputs(p, g)
            f64 = X.weighted_solve64(kS, kU, B, logm, p["W"], p["nuw"], w32[b], p["noisemodel"], r, start=starts[g])
            if f64["status"] != J.CONVERGED or f64["minz_path"] < J.MIN_Z:               # the checker's tolerance-bearing pairs: kink-free
                continue
            judged += 1
            assert out["st"][b, g] in J.INTERIOR and out["nc"][b, g] == 0, (case, b, g, out["st"][b, g])
            worst["theta"] = max(worst["theta"], J.theta_distance(out["theta"][b, g], f64))
            worst["cov"] = max(worst["cov"], J.sym_distance(unpacked(out["cov"][b, g:g + 1], D)[0], f64["inv"]))
    print(f"{case}: {judged} pairs; worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    assert judged >= ROWS * out["st"].shape[1] - 2 and all(worst[k] <= bars[k] for k in worst)


@pytest.mark.parametrize("kernel", ROW_TABLES)
def test_the_per_row_tables_are_read(kernel):
    """What keeps the row-stride layouts from being vacuous: with every row's nu, nuw and start its own, row 0 equals row 0 of the call
    whose tables are R copies of row 0's, byte for byte, and every other row differs from it."""
    case = "score_257_5_3"
    rows, copies = compact(kernel, case, "u16"), compact(kernel, case, "u16", "copies")
    first = "xy" if kernel == "kinw" else "theta"
    for k, v in outputs(rows).items():
        assert v[0].tobytes() == copies[k][0].tobytes(), k
    assert all(rows[first][b].tobytes() != copies[first][b].tobytes() for b in range(1, ROWS))
    assert all(rows["score"][b].tobytes() != copies["score"][b].tobytes() for b in range(1, ROWS))
    assert (rows["st"] != Q.NO_DATA).all() and (rows["it"] > 0).any()


# ------------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("layout", LAYOUTS, ids=names(LAYOUTS))
@pytest.mark.parametrize("kernel,case,storage", ALL, ids=ids(ALL))
def test_layout_equals_compact(kernel, case, storage, layout):
    s = spec(kernel, case, storage)
    got = L.direct_call(s, layout)
    assert got["guards_intact"] and got["outside_untouched"]
    assert got["gene_stride"] == s["M"].shape[1] + layout.pad + layout.left + layout.right
    L.assert_same_outputs(outputs(got), outputs(compact(kernel, case, storage)))


WEIGHTED_ALL = [(k, c, s) for (k, c, s) in ALL if k in WEIGHTED]
ROW_ALL = [(k, c, s) for (k, c, s) in ALL if k in ROW_TABLES]


@pytest.mark.parametrize("layout", WEIGHT_LAYOUTS, ids=names(WEIGHT_LAYOUTS))
@pytest.mark.parametrize("kernel,case,storage", WEIGHTED_ALL, ids=ids(WEIGHTED_ALL))
def test_weight_layout_equals_the_rows_of_compact(kernel, case, storage, layout):
    s = spec(kernel, case, storage)
    got = L.direct_call(s, layout)
    assert got["guards_intact"] and got["outside_untouched"] and got["weight_stride"] == s["M"].shape[1] + layout.wpad
    b0, b1 = layout.rows if layout.rows is not None else (0, ROWS)
    L.assert_same_outputs(outputs(got), {k: v[b0:b1] for k, v in outputs(compact(kernel, case, storage)).items()})


@pytest.mark.parametrize("layout", ROW_LAYOUTS, ids=names(ROW_LAYOUTS))
@pytest.mark.parametrize("kernel,case,storage", ROW_ALL, ids=ids(ROW_ALL))
def test_row_stride_layout_equals_the_rows_of_compact(kernel, case, storage, layout):
    s = spec(kernel, case, storage)
    got = L.direct_call(s, layout)
    assert got["guards_intact"] and got["outside_untouched"]
    want = compact(kernel, case, storage)
    assert all(a == (b + layout.rpad if b else 0) for a, b in zip(got["row_strides"], want["row_strides"])) and any(want["row_strides"])
    b0, b1 = layout.rows if layout.rows is not None else (0, ROWS)
    L.assert_same_outputs(outputs(got), {k: v[b0:b1] for k, v in outputs(want).items()})


@pytest.mark.parametrize("kernel,case,storage", ROW_ALL, ids=ids(ROW_ALL))
def test_one_shared_table_equals_its_copies(kernel, case, storage):
    """All row strides 0 and one table of each kind, against the call whose R tables are R copies of it."""
    s = spec(kernel, case, storage, "copies")
    got = L.direct_call(s, L.shared_tables)
    assert got["guards_intact"] and got["outside_untouched"] and not any(got["row_strides"])
    want = compact(kernel, case, storage, "copies")
    assert any(want["row_strides"])
    L.assert_same_outputs(outputs(got), outputs(want))


GENE_ALL = [(k, c, s) for (k, c, s) in ALL if k != "cell"]


@pytest.mark.parametrize("single", [False, True], ids=["inner", "single"])
@pytest.mark.parametrize("kernel,case,storage", GENE_ALL, ids=ids(GENE_ALL))
def test_gene_range_equals_the_genes_of_the_whole_call(kernel, case, storage, single):
    s = spec(kernel, case, storage)
    Ng = s["M"].shape[0]
    g0, g1 = (1, 2) if single else (1, Ng - 1)
    assert 1 <= g0 < g1 < Ng
    got = L.direct_call(s, L.gene_range(g0, g1))
    assert got["guards_intact"] and got["outside_untouched"]
    whole = outputs(compact(kernel, case, storage))
    L.assert_same_outputs(outputs(got), {k: (v[g0:g1] if kernel == "joint" else v[:, g0:g1]) for k, v in whole.items()})


CELL_ALL = [(c, s, r) for c in CASES["cell"] for s in STORAGES for r in CELL_RANGES[int(c.split("_")[1])]]


@pytest.mark.parametrize("case,storage,cells", CELL_ALL, ids=[f"{c}-{s}-{r[0]}-{r[1]}" for c, s, r in CELL_ALL])
def test_cell_range_equals_the_cells_of_the_whole_call(case, storage, cells):
    s = spec("cell", case, storage)
    c0, c1 = cells
    assert 0 < c0 < c1 <= s["M"].shape[1] and c0 % 64 and (c1 % 64 or c1 == s["M"].shape[1])
    got = L.direct_call(s, L.cell_range(c0, c1))
    assert got["guards_intact"] and got["outside_untouched"] and got["gene_stride"] == s["M"].shape[1]
    L.assert_same_outputs(outputs(got), {k: v[c0:c1] for k, v in outputs(compact("cell", case, storage)).items()})


# ------------------------------------------------------------------------------------------------------------------- row isolation
NO_DATA_FLOATS = {"kinw": ("xy", "cov", "ll", "dec", "score", "info"), "jointw": ("theta", "cov", "lls", "llu", "dec", "score", "info")}


def assert_no_data(kernel, s, got, b):
    """Row b of every gene: the header's status and outputs of a row without a usable weighted count."""
    if kernel in ROW_TABLES:
        assert (got["st"][b] == Q.NO_DATA).all() and (got["it"][b] == 0).all() and (got["nc"][b] == 0).all()
        assert all(np.isnan(got[k][b]).all() for k in NO_DATA_FLOATS[kernel])
        return
    assert (got["st"][b] == G.UNBOUNDED).all() and (got["it"][b] == 0).all()
    assert all(np.isnan(got[k][b]).all() for k in ("cov", "ll", "dec")) and (got["nu"][b][:, 1:] == 0).all()
    assert not np.isfinite(got["nu"][b][:, 0]).any()
    if kernel == "batchw":
        dm = s["args"][12][1].numpy()                                                   # delta_prior_mean_dev
        assert np.isnan(got["dvar"][b]).all() and got["delta"][b].tobytes() == np.ascontiguousarray(dm).tobytes()


@pytest.mark.parametrize("plant", ["nan_weight", "zero_row"])
@pytest.mark.parametrize("kernel,case", [("glmw", "shape_65_7_3_NegativeBinomial"), ("batchw", "silent_batch"), ("kinw", "score_257_5_3"),
                                         ("jointw", "score_257_5_3")], ids=lambda v: v)
def test_a_planted_row_ends_no_data_and_touches_no_other_row(kernel, case, plant):
    """A NaN weight, or a row of zeros, in row 1 of a call with padded weights and (where there are any) strided per-row tables: that
    row ends with the header's no-data status and outputs, and every other row equals the clean call byte for byte."""
    layout = L.both(L.row_strides(7), L.weights_padded(61)) if kernel in ROW_TABLES else L.weights_padded(61)
    clean = L.direct_call(spec(kernel, case, "u16"), layout)
    Wt = weights(kernel, case)
    if plant == "nan_weight":
        Wt[1, 17] = np.nan
    else:
        Wt[1] = 0.0
    s = spec(kernel, case, "u16", "layout", as_tuple(Wt))
    got = L.direct_call(s, layout)
    assert got["guards_intact"] and got["outside_untouched"] and clean["guards_intact"]
    assert_no_data(kernel, s, got, 1)
    for k, v in outputs(clean).items():
        assert got[k][0].tobytes() == v[0].tobytes() and got[k][2].tobytes() == v[2].tobytes(), k
    L.assert_same_outputs(outputs(clean), outputs(compact(kernel, case, "u16")))


# ---------------------------------------------------------------------------------------------------------- the 32-bit row indices
def big_spec(kernel):
    case = BIG_CASES[kernel]
    s = spec(kernel, case, "u16")
    return s if kernel == "cell" else L.take_genes(s, 0, L.BIG_NG)


@pytest.mark.parametrize("kernel", list(BIG_CASES))
def test_row_index_beyond_32_bits(kernel, big):                                         # noqa: F811
    """uint16, Ng = 3, Nc = 257, gene_stride = 2^30 + 1, counts_dev 2^31 elements into the allocation (the joint kernels: U's rows 300
    elements behind S's): 2 gene_stride does not fit a signed 32-bit integer, and what a truncated index addresses is inside the
    allocation and poison (tests/test_cabi_layouts_cpu.py)."""
    s = big_spec(kernel)
    assert s["M"].shape == (L.BIG_NG, L.BIG_NC) and s["M"].dtype == np.uint16
    want = L.direct_call(s, L.compact)
    got = L.direct_call(s, L.big_stride, big=big)
    assert got["gene_stride"] == 2 ** 30 + 1 and got["guards_intact"] and want["guards_intact"]
    L.assert_same_outputs(outputs(got), outputs(want))


@pytest.fixture(scope="module")
def big_weights():
    """One allocation for the four tests: 2^31 + 2 weight_stride + Nc float32 elements, every byte 0xFF; freed when the module is done."""
    free, _ = torch.cuda.mem_get_info()
    if free < L.BIGW_FREE_NEEDED:
        pytest.skip(f"the 32-bit weight-row tests need {L.BIGW_FREE_NEEDED} bytes free on the device ({4 * L.BIGW_TOTAL} in one allocation); "
                    f"{free} are free")
    t = L.big_weight_allocation(dev())
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", WEIGHTED)
def test_weight_row_index_beyond_32_bits(kernel, big_weights):
    """R = 3, Nc = 257, weight_stride = 2^30 + 1, weights_dev 2^31 floats into an allocation of NaN: 2 weight_stride does not fit a signed
    32-bit integer, and what a truncated index addresses is inside the allocation and NaN (tests/test_cabi_layouts_cpu.py)."""
    s = big_spec(kernel)
    assert L.weights_of(s).shape == (L.BIGW_ROWS, L.BIG_NC)
    want = L.direct_call(s, L.compact)
    got = L.direct_call(s, L.big_weight_stride, big=big_weights)
    assert got["weight_stride"] == 2 ** 30 + 1 and got["guards_intact"] and want["guards_intact"]
    L.assert_same_outputs(outputs(got), outputs(want))
