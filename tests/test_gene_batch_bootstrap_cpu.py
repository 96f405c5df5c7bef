"""CPU: the checker of the weighted batch-aware per-gene fit (tests/gene_batch_boot_checker.py) against itself, the bootstrap estimator on
the float64 reference, the host-side refusals of `gene_harmonics_batched_bootstrap` and `gene_harmonics_batched(cell_weights=)`, the
summaries of `GeneBatchHarmonicBootstrap`, the C entry point's refusals and the kernel's code object (no scratch)."""
import ctypes as C
import inspect
import os
import re
import subprocess
from dataclasses import fields

import numpy as np
import pytest

from tests import gene_batch_boot_checker as Q
from tests import gene_batch_checker as BC
from tests import gene_glm_checker as G
from velocycle_amd.gene_batch import GeneBatchHarmonicFit, gene_harmonics_batched
from velocycle_amd.gene_bootstrap import GeneBatchHarmonicBootstrap, GeneHarmonicBootstrap, gene_harmonics_batched_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_pair_is_left_out():
    """With these weights the float64 reference and its null model converge for every (row, gene) pair of every case: the bars hold all
    of them.  The drawn rows empty the one-cell batch in 2 of the 4 rows of the seven_* cases and of one_and_1000, and the hand-made row
    empties the last batch: those paths are held to the bars, not only to a status."""
    assert Q.left_out_share() == 0.0
    assert set(Q.cases()) == set(Q.DRAWN) | {Q.EMPTY_LAST, Q.UNIFORM}
    for name in Q.DRAWN:
        p, Wt = Q.cases()[name]
        assert Wt.shape == (4, p["S"].shape[0]) and Q.is_integer(name)
        if name.startswith("seven_") or name == "one_and_1000":
            assert list(Q.emptied(name)[:, 0]).count(True) == 2 and not Q.emptied(name)[:, 1:].any(), name
    last = Q.emptied(Q.EMPTY_LAST)
    assert last.shape == (1, 3) and list(last[0]) == [False, False, True]
    assert not Q.is_integer(Q.UNIFORM) and Q.solved(Q.UNIFORM)[0][0][2] is None
    # the expansion that empties the last batch keeps its coefficient (prior mean 0, its variance the prior's)
    f64 = Q.solved(Q.EMPTY_LAST)[0][0][0]
    assert f64["nu"].shape == (3 + 3,) and abs(f64["nu"][-1]) <= 1e-12 and abs(f64["std"][-1] ** 2 - 0.25) <= 0.25


def test_bars_are_finite_and_capped():
    bars = Q.bars()
    print("bars:", bars)
    assert set(bars) == set(BC.YARDSTICKS)
    assert all(np.isfinite(v) and v > 0 for v in bars.values()), bars
    assert bars["coef"] <= G.COEF_CAP, bars


def test_expansion_equals_the_written_out_weighted_newton():
    """On integer weights the two references are the same fit, on every integer-weight case (emptied batches among them): the same
    log-likelihood and Hessian, and coefficients within the two stopping rules.  Each iteration stops at a decrement
    dec <= 1e-24 max(1, |objective|), that is within sqrt(dec) standard errors of the optimum, so the two lie within
    2e-12 sqrt(max(1, sum |log p|)) standard errors of each other (sum |log p| >= |objective| up to the penalty); measured worst
    4.1e-11, in the large-count cases."""
    worst = 0.0
    for name, (p, Wt) in Q.cases().items():
        if not Q.is_integer(name):
            continue
        for b, w in enumerate(Wt):
            for g in range(p["S"].shape[1]):
                k, B, lab, logm, r, prior, dprior = BC.gene_inputs(p, g)
                f64 = Q.solved(name)[b][g][0]
                wn = Q.written_out64(k, B, lab, logm, w, p["noisemodel"], r, prior, dprior)
                assert wn["status"] == G.CONVERGED and f64["status"] == G.CONVERGED
                d = wn["nu"] - f64["nu"]
                dist = float(np.sqrt(max(d @ f64["hess"] @ d, 0.0)))
                worst = max(worst, dist)
                assert dist <= 2e-12 * np.sqrt(max(1.0, f64["abs"])), (name, b, g, dist)
                assert abs(wn["loglik"] - f64["loglik"]) <= 1e-10 * f64["abs"], (name, b, g)
                assert np.allclose(wn["hess"], f64["hess"], rtol=1e-9, atol=1e-12)
    print("worst distance, standard errors:", worst)


def test_the_restatement_from_either_start_ends_within_its_steps():
    for name in Q.cases():
        if not Q.is_integer(name):
            continue
        for row in Q.solved(name):
            for (f64, n64, f32, n32, f32w) in row:
                assert f32["status"] in (G.CONVERGED, G.ROUNDING) and f32w["status"] in (G.CONVERGED, G.ROUNDING), name
                assert n32["status"] in (G.CONVERGED, G.ROUNDING), name
                assert f32["nu"].shape == f64["nu"].shape == f32w["nu"].shape


def test_the_bootstrap_widens_the_harmonics_stds_of_a_poisson_fit_with_batches():
    """Three batches of 200 cells, negative-binomial counts (shape_inv 0.3), gene 0, H = 1, Poisson fit with offsets, 200 Poisson(1)
    resamples, float64 reference only.  On the sine and cosine coefficients the bootstrap is at least 1.15 x wider than the Hessian
    (measured: 1.87 and 2.04).  nu_0 and the offsets are NOT compared that way: the likelihood fixes only nu_0 + delta_b, their split is
    the offsets' prior, so their Hessian stds hold the prior's width while the resamples see the sampling spread alone (ratio 0.09
    for nu_0, 0.13 to 0.15 for the offsets, recorded only).  What the data does fix, nu_0 + delta_b, is again wider under the
    bootstrap (measured 1.99 to 2.19)."""
    sim = BC.simulated((200, 200, 200), 2, seed=21, level=2.0)
    k, B, lab, logm = np.trunc(sim["S"][:, 0]), G.basis64(sim["phis"], 1), sim["labels"], np.log(sim["n"])
    full = BC.newton64(k, B, lab, logm, "Poisson")
    assert full["status"] == G.CONVERGED
    Wt = np.random.default_rng(7).poisson(1, (200, 600)).astype(np.float64)
    reps = []
    for w in Wt:
        f = Q.reference64(k, B, lab, logm, w, "Poisson", None, None, BC.DELTA_PRIOR)
        assert f["status"] == G.CONVERGED
        reps.append(f["nu"])
    reps = np.array(reps)
    ratio = np.std(reps, axis=0, ddof=1) / full["std"]
    level = np.array([np.std(reps[:, 0] + reps[:, 3 + b], ddof=1) / np.sqrt(full["cov"][0, 0] + full["cov"][3 + b, 3 + b] + 2 * full["cov"][0, 3 + b])
                      for b in range(3)])
    print("std_boot / std_hess [nu0, sin, cos, delta x 3]:", ratio, " of nu0 + delta_b:", level)
    assert (ratio[1:3] >= 1.15).all(), ratio
    assert (level >= 1.15).all(), level


def _inputs(Nc=6, Ng=2):
    return np.ones((Nc, Ng), np.float32), G.directions(np.arange(float(Nc))), np.ones(Nc), np.array([0, 1, 0, 1, 0, 1])


def test_host_refusals_of_the_bootstrap_worker():
    S, xy, n, lab = _inputs()
    for bad in ("mle", "other"):
        with pytest.raises(ValueError, match="dispersion"):
            gene_harmonics_batched_bootstrap(S, xy, n, lab, noisemodel="NegativeBinomial", dispersion=bad)
    for bad in (0, 65536, 2.5):
        with pytest.raises(ValueError, match="n_boot"):
            gene_harmonics_batched_bootstrap(S, xy, n, lab, n_boot=bad)
    with pytest.raises(ValueError, match="1 GiB"):
        gene_harmonics_batched_bootstrap(np.ones((2, 30000), np.float32), G.directions(np.arange(2.0)), np.ones(2), np.array([0, 1]),
                                         harmonics=3, n_boot=500)                    # 500 x (7 + 2) x 30000 x 8 bytes
    for bad in (np.full((3, 6), -1.0), np.full((3, 6), np.nan), np.full((3, 6), np.inf), np.ones((3, 5)), np.ones(6)):
        with pytest.raises(ValueError, match="weights"):
            gene_harmonics_batched_bootstrap(S, xy, n, lab, weights=bad)
    with pytest.raises(NotImplementedError):
        gene_harmonics_batched_bootstrap(S, xy, n, lab, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="no cell"):
        gene_harmonics_batched_bootstrap(S, xy, n, np.array([0, 2, 0, 2, 0, 2]))
    with pytest.raises(ValueError, match="fit.means"):
        gene_harmonics_batched_bootstrap(S, xy, n, lab, fit=type("F", (), {"means": np.zeros((3, 2)), "delta_nu": np.zeros((3, 2))})())
    sig = inspect.signature(gene_harmonics_batched_bootstrap)
    assert [(q.name, q.default) for q in sig.parameters.values() if q.kind == q.KEYWORD_ONLY] == [
        ("n_boot", 200), ("seed", 0), ("weights", None), ("fit", None), ("delta_nu_prior", (0.0, 0.5)), ("prior_means", None),
        ("prior_stds", None), ("tol", 1e-10), ("max_iter", 25), ("device", None), ("chunk_genes", None), ("storage", "auto"),
        ("return_weights", False)]
    assert [q.name for q in sig.parameters.values() if q.kind == q.POSITIONAL_OR_KEYWORD] == [
        "counts", "directions", "n_scounts", "batches", "harmonics", "a", "noisemodel", "dispersion"]


def test_cell_weights_go_by_name_and_other_names_are_refused():
    S, xy, n, lab = _inputs()
    with pytest.raises(TypeError, match="cell_weight"):
        gene_harmonics_batched(S, xy, n, lab, cell_weight=np.ones(6))
    with pytest.raises(TypeError, match="bootstrap"):
        gene_harmonics_batched(S, xy, n, lab, bootstrap=4)
    for bad in (np.ones(5), np.ones((1, 6)), np.full(6, -1.0), np.full(6, np.nan)):
        with pytest.raises(ValueError, match="weights"):
            gene_harmonics_batched(S, xy, n, lab, cell_weights=bad)
    kinds = {q.name: q.kind for q in inspect.signature(gene_harmonics_batched).parameters.values()}
    assert kinds["options"] == inspect.Parameter.VAR_KEYWORD and "cell_weights" not in kinds
    assert "bootstrap" not in [f.name for f in fields(GeneBatchHarmonicFit)] and GeneBatchHarmonicFit.bootstrap is None
    import velocycle_amd
    assert velocycle_amd.gene_harmonics_batched_bootstrap is gene_harmonics_batched_bootstrap
    assert velocycle_amd.GeneBatchHarmonicBootstrap is GeneBatchHarmonicBootstrap
    assert {"gene_harmonics_batched_bootstrap", "GeneBatchHarmonicBootstrap"} <= set(velocycle_amd.__all__)


def test_summaries_on_a_hand_made_replicate_array():
    # 4 replicates, H = 0, 2 batches, 3 genes: gene 0 has three ok replicates, gene 1 one, gene 2 none
    rep = np.zeros((4, 1, 3))
    rep[:, 0, 0] = [1.0, 2.0, 3.0, 100.0]
    dl = np.zeros((4, 2, 3))
    dl[:, 0, 0] = [0.5, 1.5, 2.5, -50.0]
    dl[:, 1, 0] = [1.0, 1.0, 4.0, np.nan]
    dl[:, :, 1] = [[5.0, 3.0], [np.nan, np.nan], [-np.inf, 0.0], [7.0, 7.0]]
    dl[:, :, 2] = np.nan
    status = np.array([[0, 0, 2], [1, 3, 2], [0, 2, 4], [4, 4, 3]], dtype=np.int32)
    fit = type("F", (), {"means": np.ones((1, 3)), "delta_nu": np.full((2, 3), 0.5)})()
    bs = GeneBatchHarmonicBootstrap(rep, status, np.zeros((4, 3), np.int32), fit=fit, delta_replicates=dl)
    assert isinstance(bs, GeneHarmonicBootstrap) and bs.harmonics == 0 and list(bs.n_ok) == [3, 1, 0]
    assert np.allclose(bs.means[:, 0], [2.0]) and np.allclose(bs.stds[:, 0], [1.0])          # the coefficients: the base class's
    assert np.allclose(bs.delta_nu_means[:, 0], [1.5, 2.0]) and np.array_equal(bs.delta_nu_means[:, 1], [5.0, 3.0])
    assert np.isnan(bs.delta_nu_means[:, 2]).all()
    assert np.allclose(bs.delta_nu_stds[:, 0], np.std(dl[:3, :, 0], axis=0, ddof=1))          # ddof 1 over the ok replicates only
    assert np.isnan(bs.delta_nu_stds[:, 1]).all() and np.isnan(bs.delta_nu_stds[:, 2]).all()  # below 2 ok replicates
    assert np.allclose(bs.delta_nu_bias[:, 0], [1.0, 1.5])
    lo, hi = bs.delta_nu_interval(0.5)
    assert np.allclose(lo[:, 0], np.quantile(dl[:3, :, 0], 0.25, axis=0)) and np.allclose(hi[:, 0], np.quantile(dl[:3, :, 0], 0.75, axis=0))
    assert np.array_equal(lo[:, 1], [5.0, 3.0]) and np.isnan(lo[:, 2]).all()
    with pytest.raises(ValueError):
        bs.delta_nu_interval(1.0)
    assert [f.name for f in fields(bs)] == [f.name for f in fields(GeneHarmonicBootstrap)] + ["delta_replicates"]


def batch_boot_args(**k):
    """Arguments of vc_gene_glm_batch_weighted with pointers that are never dereferenced (seg_host is host memory and real): every call
    made with them is refused before the launch."""
    one = C.c_void_p(64)
    seg = (C.c_int64 * 3)(*k.get("seg", (0, 2, 4)))
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("noise", 1), k.get("r", None), k.get("Nb", 2), None if k.get("no_seg") else seg, k.get("dm", one),
            k.get("dq", one), k.get("pm", None), k.get("pp", None), k.get("weights", one), k.get("R", 2), k.get("wstride", 4),
            k.get("start_nu", None), k.get("start_delta", None), k.get("tol", 1e-10), k.get("max_iter", 25), k.get("nu", one),
            k.get("delta", one), k.get("cov", None), k.get("dvar", None), k.get("ll", one), k.get("dec", one), k.get("it", one),
            k.get("st", one), None]


REFUSALS = [(dict(K=2), b"K must be"), (dict(Nc=0), b"Ng and Nc"), (dict(stride=3), b"gene_stride"), (dict(max_iter=0), b"max_iter"),
            (dict(tol=-1.0), b"tol"), (dict(Nb=0), b"Nb must be"), (dict(Nb=33), b"Nb must be"), (dict(counts=None), b"null input"),
            (dict(no_seg=True), b"null input"), (dict(dm=None), b"needs its prior"), (dict(nu=None), b"null output"),
            (dict(delta=None), b"null output"), (dict(st=None), b"null output"), (dict(noise=0), b"r_dev"),
            (dict(pm=C.c_void_p(64)), b"prior of nu"), (dict(seg=(1, 2, 4)), b"seg must start"), (dict(seg=(0, 2, 3)), b"seg must start"),
            (dict(seg=(0, 5, 4)), b"non-decreasing"), (dict(seg=(0, 0, 4)), b"empty segment"),
            (dict(weights=None), b"null weights_dev"), (dict(R=0), b"R must be"), (dict(R=65536), b"R must be"),
            (dict(wstride=3), b"weight_stride"), (dict(start_nu=C.c_void_p(64)), b"start_nu_dev and start_delta_dev"),
            (dict(start_delta=C.c_void_p(64)), b"start_nu_dev and start_delta_dev"), (dict(cov=C.c_void_p(64)), b"cov_nu_dev and delta_var_dev"),
            (dict(dvar=C.c_void_p(64)), b"cov_nu_dev and delta_var_dev")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    for kw, msg in REFUSALS:
        assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), (kw, lib.vc_last_error(None))
        assert lib.vc_last_error(None).startswith(b"vc_gene_glm_batch_weighted: ")
    # the order: vc_gene_glm_batch's refusals come before the new ones
    assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(seg=(0, 0, 4), weights=None, R=0)) == _lib.VC_ERR_ARG
    assert b"empty segment" in lib.vc_last_error(None)
    assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(weights=None, R=0, wstride=3)) == _lib.VC_ERR_ARG
    assert b"null weights_dev" in lib.vc_last_error(None)
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_glm_batch_weighted.hip")).read()
    body = src[src.index('extern "C" int vc_gene_glm_batch_weighted'):]
    launch = body.index("hipLaunchKernelGGL")                                            # every refusal comes before the launch
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < body.rindex("gene_fail(") < launch
    header = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert "int vc_gene_glm_batch_weighted(" in header and "#define VC_ABI_VERSION 2" in header
    assert " *   vc_gene_glm_batch_weighted " in header                                          # the list at the head of the file


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_gene_glm_batch_weighted_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly
    emitted for gfx950 (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_glm_batch_weighted.hip")
    out = str(tmp_path / "glmbw.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    found = re.findall(r"\.name:\s+(\S*vc_gene_glm_batch_weighted_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    assert len(found) == 16, len(found)                    # H 0..3 x {Poisson, NB} x {u16, f32}
    assert all(int(p) == 0 for _, p in found), found
