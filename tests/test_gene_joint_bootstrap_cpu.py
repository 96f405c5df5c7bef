"""CPU: the checker of the weighted joint fit (tests/gene_joint_boot_checker.py) against itself, the calibration of the bootstrap
standard error of the speed ratio on the float64 outer checker, the header and binding of vc_gene_joint_weighted, its refusals and its
code object, the host-side refusals of `gene_joint_weighted` and `velocity_map_joint_bootstrap`, the summaries of
`JointVelocityMapBootstrap` and the containers' plumbing."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

from tests import gene_joint_boot_checker as X
from tests import gene_joint_checker as Q
from tests.gene_kinetics_checker import simulate
from tests.test_gene_joint_cpu import REFUSALS as PLAIN_REFUSALS
from velocycle_amd.gene_joint import GeneJointFit, JointVelocityMapFit, check_arguments, velocity_map_joint
from velocycle_amd.joint_bootstrap import (GeneJointBootstrap, JointVelocityMapBootstrap, gene_joint_bootstrap, gene_joint_weighted,
                                           velocity_map_joint_bootstrap)
from velocycle_amd.kinetics_bootstrap import VelocityMapBootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the checker
def test_warm_start_pairs_are_kink_free_and_converged():
    """Seed 22, 3 rows, all 18 cases from the float64 fit of the unweighted data: every pair kink-free (min z >= MIN_Z at every point
    the reference evaluates) and CONVERGED, the restatement CONVERGED / ROUNDING; the reference takes at most 8 steps, the restatement
    7.  The only cell of shape_1_1_1_Poisson drew weight 0 in all three rows: those three are the NO_DATA pairs."""
    total = sum(len(row) for name in X.PAIR_CASES for row in X.solved_warm(name))
    assert total == 3 * sum(Q.cases()[name]["U"].shape[1] for name in X.PAIR_CASES) and len(X.PAIR_CASES) == 18
    lost = X.left_out(X.solved_warm, X.PAIR_CASES)
    assert lost == {("shape_1_1_1_Poisson", b, 0) for b in range(3)} and (X.weights("shape_1_1_1_Poisson") == 0).all(), lost
    steps64 = steps32 = 0
    for name in X.PAIR_CASES:
        rows = X.solved_warm(name)
        X.assert_kink_free(name, rows)
        for row in rows:
            for s in row:
                if s is not None:
                    assert s[1]["status"] in Q.INTERIOR and s[1]["minz_path"] >= Q.MIN_Z, name
                    steps64, steps32 = max(steps64, s[0]["iterations"]), max(steps32, s[1]["iterations"])
    print("steps: reference", steps64, "restatement", steps32)
    assert steps64 <= 8 and steps32 <= 7


def test_default_start_pairs_are_kink_free_and_the_restatement_stops_with_the_reference():
    """The 15 cases that carry a tolerance from the default start, each under the first weight seed in 11..40 for which every pair is
    kink-free; the restatement stops within a step of where the reference's decrement first falls to the device's tolerance."""
    assert set(X.DEFAULT_SEEDS) | set(X.NO_DEFAULT_TOLERANCE) == set(X.PAIR_CASES) and len(X.DEFAULT_SEEDS) == 15
    lost = X.left_out(X.solved_default, list(X.DEFAULT_SEEDS))
    assert lost == {("shape_1_1_1_Poisson", 0, 0), ("shape_1_1_1_Poisson", 2, 0)}, lost
    for name in X.DEFAULT_SEEDS:
        rows = X.solved_default(name)
        X.assert_kink_free(name, rows)
        for row in rows:
            for s in row:
                if s is not None:
                    assert s[1]["status"] in Q.INTERIOR and abs(s[1]["iterations"] - s[0]["first_tol"]) <= 1, (name, s[1]["iterations"])


def test_bars_are_finite():
    bars = X.bars()
    print("bars:", bars)
    print("unweighted bars:", Q.bars())
    keys = set(Q.bars()) - {"steps"}
    assert set(bars) == keys | {"steps_warm", "steps_default"} and all(np.isfinite(bars[k]) and bars[k] > 0 for k in keys), bars


def test_expansion_equals_the_written_out_weighted_formulas():
    """On integer weights the two references are the same fit: the optimum within 1e-8 standard errors, and at two points every figure
    (objectives, gradient, the step's matrix, score, information) to rounding; the rounding scales and the clamped count differ as
    documented (a repeated cell weighs wt^2 in N, and is one cell in n_clamped)."""
    name = X.UNIFORM_CASE
    p, Wt = Q.cases()[name], X.weights(name)
    worst, clamped = 0.0, 0
    for b, w in enumerate(Wt):
        pe = X.expand(p, w)
        for g in range(p["U"].shape[1]):
            kS, kU, B, logm, r = Q.gene_inputs(p, g)
            f64 = X.solved_warm(name)[b][g][0]
            ws = X.weighted_solve64(kS, kU, B, logm, p["W"], p["nuw"], w, p["noisemodel"], r, start=X.warm_starts(name)[g])
            assert ws["status"] == Q.CONVERGED
            worst = max(worst, Q.theta_distance(ws["th"], f64))
            assert abs(ws["L_S"] - f64["L_S"]) <= 1e-10 * f64["abs_S"] and np.allclose(ws["inv"], f64["inv"], rtol=1e-7, atol=0)
            kSe, kUe, Be, le, re_ = Q.gene_inputs(pe, g)
            for at in Q.evaluate_points(p, g)[1:4:2] + Q.evaluate_points(p, g)[4:]:          # the last point clamps cells
                a = X.weighted_point64(at, kS, kU, B, logm, p["W"], p["nuw"], w, p["noisemodel"], r)
                e = Q.point64(at, kSe, kUe, Be, le, pe["W"], p["nuw"], p["noisemodel"], re_)
                assert a["observed"] == e["observed"]
                scale = e["abs_S"] + e["abs_U"]
                for key in ("L_S", "L_U", "f", "A", "abs_S", "abs_U", "G", "M", "F", "score", "info", "dec"):
                    assert np.allclose(a[key], e[key], rtol=1e-9, atol=1e-9 * scale), (b, g, key, a[key], e[key])
                assert (a["N"] >= e["N"] * (1 - 1e-12)).all() and (a["N"] <= w.max() * e["N"] * (1 + 1e-12)).all()
                assert a["n_clamped"] <= e["n_clamped"] and (a["n_clamped"] > 0) == (e["n_clamped"] > 0)
                clamped += a["n_clamped"]
    assert clamped > 0
    print("worst distance, standard errors:", worst)
    assert worst <= 1e-8
    for row in X.solved_uniform():                                           # the non-integer table has a reference everywhere
        assert all(s["status"] == Q.CONVERGED and s["minz_path"] >= Q.MIN_Z for s in row)
    kS, kU, B, logm, r = Q.gene_inputs(p, 0)                                 # the default start of the weighted formulas is the expansion's
    kSe, kUe, Be, le, _ = Q.gene_inputs(X.expand(p, Wt[0]), 0)
    prior = Q.prior_of(B.shape[0])
    assert np.allclose(X.weighted_start(kS, kU, B, logm, p["W"], p["nuw"], Wt[0], prior),
                       Q.start_theta(kSe, kUe, Be, le, X.expand(p, Wt[0])["W"], p["nuw"], prior), rtol=1e-13)


def test_weighted_gradient_and_matrices_by_finite_differences():
    """Non-integer weights: G is the gradient of f, O minus the second derivative of f (central differences), and the score the
    derivative of f in nuw, at a kink-free point."""
    p = Q.cases()[X.UNIFORM_CASE]
    w = X.uniform_weights()[0]
    kS, kU, B, logm, r = Q.gene_inputs(p, 1)
    f = lambda th, nuw=p["nuw"]: X.weighted_point64(th, kS, kU, B, logm, p["W"], nuw, w, p["noisemodel"], r)      # noqa: E731
    th = Q.truth(p, 1) + 0.01
    at = f(th)
    assert at["minz"] >= Q.MIN_Z and at["observed"]
    h = 1e-5
    D = len(th)
    G = np.array([(f(th + h * e)["f"] - f(th - h * e)["f"]) / (2 * h) for e in np.eye(D)])
    H = np.array([(f(th + h * e)["G"] - f(th - h * e)["G"]) / (2 * h) for e in np.eye(D)])
    S = np.array([(f(th, p["nuw"] + h * e)["f"] - f(th, p["nuw"] - h * e)["f"]) / (2 * h) for e in np.eye(len(p["nuw"]))])
    print("gradient", np.abs(G - at["G"]).max(), "observed", np.abs(H + at["O"]).max() / np.abs(at["O"]).max(), "score", np.abs(S - at["score"]).max())
    assert np.allclose(G, at["G"], rtol=1e-6, atol=1e-5 * np.abs(at["G"]).max() + 1e-4)
    assert np.allclose(-H, at["O"], rtol=1e-6, atol=1e-6 * np.abs(at["O"]).max())
    assert np.allclose(S, at["score"], rtol=1e-6, atol=1e-4)


def test_outer_cases_as_stated():
    """Both outer cases under 2 rows of seed 22, warm at the full-data reference: all four replicates CONVERGED in 3 reference rounds
    and 2 of the restatement, no gene excluded, least min z over the traces 0.329 and 0.387, the restatement within 6.7e-5 reference
    standard errors (measured: 3.4e-6 .. 4.4e-5), the replicates 0.01 .. 0.35 standard errors from the full-data fit (measured:
    0.0075 .. 0.346, held to 0.007 .. 0.36)."""
    least = {}
    for name in Q.OUTER_CASES:
        full = Q.outer_solved(name)[0]
        rows = X.outer_solved(name)
        assert len(rows) == X.OUTER_ROWS
        for m64, m32, trace in rows:
            d = m32["nuw"] - m64["nuw"]
            moved = np.abs(m64["nuw"] - full["nuw"]) / full["std"]
            print(name, m64["status"], m64["rounds"], m32["rounds"], min(z for _, z in trace), math.sqrt(d @ m64["J"] @ d), moved)
            assert m64["status"] == m32["status"] == "CONVERGED" and m64["rounds"] == 3 and m32["rounds"] == 2
            assert m64["n_excluded"] == m32["n_excluded"] == 0 and math.sqrt(d @ m64["J"] @ d) <= 6.7e-5
            assert 0.007 <= moved.min() and moved.max() <= 0.36
            least[name] = min(least.get(name, math.inf), min(z for _, z in trace))
    assert abs(least["outer_3000_40"] - 0.329) < 1e-3 and abs(least["outer_1500_30"] - 0.387) < 1e-3, least


def _log_ratio_se(m):
    v, c = m["nuw"], m["cov"]
    return math.sqrt(c[0, 0] / v[0] ** 2 + c[1, 1] / v[1] ** 2 - 2 * c[0, 1] / (v[0] * v[1]))


def test_the_bootstrap_sees_what_the_laplace_error_of_a_poisson_fit_misses():
    """Negative-binomial counts (r = 3), two conditions, outer_1500_30's settings cut to 1500 cells x 8 genes so that the float64 outer
    checker runs 16 integer-weight rows per noise model in seconds: simulate(41, 1500, 8, 1, NB, [0.45, 0.3], Nx=2, level=(4.0, 5.5))
    with S drawn from its own nu, Poisson(1) rows from default_rng(12), each replicate `outer_from` (float64) on the cell-expanded data
    started at the full fit.  The ratio of the bootstrap standard deviation of ln(omega_0 / omega_1) to its Laplace error is larger
    under the Poisson fit (misspecified) than under the negative-binomial fit (measured: see profiles/r23_gene_joint_bootstrap.md)."""
    p = Q.with_spliced(simulate(41, 1500, 8, 1, Q.NB, [0.45, 0.3], Nx=2, level=(4.0, 5.5)), 41)
    Wt = np.random.default_rng(12).poisson(1, (16, 1500))
    ratio = {}
    for noise, prob in ((Q.NB, p), (Q.PO, dict(p, noisemodel=Q.PO, r=None))):
        full = Q.map64(prob)
        assert full["status"] == "CONVERGED"
        starts, reps = [f["th"] for f in full["fits"]], []
        for w in Wt:
            m = X.outer_from(X.expand(prob, w), Q.solve64, lambda f: f["status"] == Q.CONVERGED, 1e-14, 60, 8 * Q.EPS64, full["nuw"], starts)
            assert m["status"] == "CONVERGED"
            reps.append(math.log(m["nuw"][0] / m["nuw"][1]))
        ratio[noise] = np.std(reps, ddof=1) / _log_ratio_se(full)
        print(f"{noise} fit: bootstrap sd {np.std(reps, ddof=1):.4f}, Laplace se {_log_ratio_se(full):.4f}, ratio {ratio[noise]:.2f}")
    assert ratio[Q.PO] > ratio[Q.NB], ratio


# ---------------------------------------------------------------------------------------------------------------- the C side
def test_header_declares_and_lib_binds_vc_gene_joint_weighted():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert " *   vc_gene_joint_weighted " in hdr and "#define VC_ABI_VERSION 2" in hdr
    decl = re.search(r"\bint vc_gene_joint_weighted\(([^;]*)\);", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert len(_lib.EXPORTS["vc_gene_joint_weighted"][1]) == len(names) == 36 and names[-1] == "hip_stream"
    plain = [a.split()[-1].lstrip("*") for a in re.search(r"\bint vc_gene_joint\(([^;]*)\);", hdr).group(1).split(",")]
    added = ["nuw_row_stride", "weights_dev", "R", "weight_stride", "start_row_stride"]
    assert [n for n in names if n not in added] == plain and [n for n in names if n in added] == added
    types = _lib.EXPORTS["vc_gene_joint_weighted"][1]
    assert all(types[names.index(n)] is (C.c_void_p if n == "weights_dev" else C.c_int64) for n in added)
    assert [t for n, t in zip(names, types) if n not in added] == _lib.EXPORTS["vc_gene_joint"][1]
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint_weighted.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace {")[1]
    assert f"JNTW_BOUND = {Q.XY_BOUND};" in src and f"JNTW_MAX_HALVINGS = {Q.HALVINGS};" in src and "JNTW_FLOOR = 1.0e-5;" in src
    assert "JNTW_SLAB = 65535;" in src and "JNTW_MAX_ROWS = 65535;" in src
    assert '#include "vc_gene_glm_math.h"' in src and src.count("#include") == 1


def jntw_args(**k):
    """Arguments of vc_gene_joint_weighted with pointers that are never dereferenced: every call made with them is refused before the
    launch."""
    one = C.c_void_p(64)
    return [k.get("counts_s", one), k.get("counts_u", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4),
            k.get("basis", one), k.get("K", 3), k.get("logm", one), k.get("w", one), k.get("NW", 1), k.get("nuw", one), k.get("nuw_stride", 0),
            k.get("noise", 1), k.get("r", None), k.get("pm", one), k.get("pp", one), k.get("prior", one), k.get("weights", one), k.get("R", 2),
            k.get("wstride", 4), k.get("start", None), k.get("start_stride", 0), k.get("tol", 1e-10), k.get("max_iter", 25),
            k.get("theta", one), k.get("cov", one), k.get("lls", one), k.get("llu", one), k.get("dec", one), k.get("it", one),
            k.get("st", one), k.get("nc", one), k.get("score", one), k.get("info", one), None]


# vc_gene_joint's refusals (cov_dev may be NULL here), then the weighted entry point's own
REFUSALS = [(kw, msg) for kw, msg in PLAIN_REFUSALS if kw != dict(cov=None)] + \
    [(dict(weights=None), b"null weights_dev"), (dict(R=0), b"R must be"), (dict(R=65536), b"R must be"), (dict(wstride=3), b"weight_stride"),
     (dict(nuw_stride=2, NW=3), b"nuw_row_stride"), (dict(nuw_stride=-1), b"nuw_row_stride"),
     (dict(start=C.c_void_p(64), start_stride=19), b"start_row_stride"), (dict(start=C.c_void_p(64), start_stride=-20), b"start_row_stride")]
# the order: a shared refusal wins over an own one, vc_gene_joint's over the weights'
ORDER = [(dict(K=2, weights=None), b"K must be"), (dict(counts_s=None, weights=None), b"null input"), (dict(weights=None, R=0), b"null weights_dev"),
         (dict(R=0, wstride=3), b"R must be"), (dict(wstride=3, nuw_stride=-1), b"weight_stride"), (dict(max_iter=0, weights=None), b"start_dev")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert len(REFUSALS) == len(PLAIN_REFUSALS) - 1 + 8
    for kw, msg in REFUSALS + ORDER:
        assert lib.vc_gene_joint_weighted(*jntw_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), (kw, lib.vc_last_error(None))
        assert lib.vc_last_error(None).startswith(b"vc_gene_joint_weighted: ")
    assert lib.vc_gene_joint_weighted(*jntw_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint_weighted.hip")).read()
    body = src[src.index('extern "C" int vc_gene_joint_weighted('):]
    launch = body.index("hipLaunchKernelGGL")
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < launch
    assert body.rindex("gene_fail(") < launch < body.index("gene_launched(")


def test_the_code_object(tmp_path):
    """All 32 instantiations of vc_gene_joint_weighted_kernel (H {1, 2} x NW 0..3 x {NB, Poisson} x {u16, f32}) in the assembly emitted
    for gfx950: .private_segment_fixed_size 0 (no scratch), vc_gene_joint's LDS (1160 .. 2320 bytes) and at most 512 VGPRs (measured
    202 .. 282, accumulation registers included; vc_gene_joint's own are 200 .. 300)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint_weighted.hip")
    out = str(tmp_path / "jntw.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*vc_gene_joint_weighted_kernel\S*)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(found) == 32 and len({name for _, name, _, _ in found}) == 32, len(found)
    print("VGPRs:", sorted({int(v) for _, _, _, v in found}), "LDS:", sorted({int(lds) for lds, _, _, _ in found}))
    assert all(int(p) == 0 for _, _, p, _ in found), found
    assert all(int(v) <= 512 for _, _, _, v in found), found
    assert {int(lds) for lds, _, _, _ in found} == {5 * 8 * n for n in (29, 30, 39, 46, 47, 58)}


# ---------------------------------------------------------------------------------------------------------------- the Python side
def small(Nc=6, Ng=2):
    return np.ones((Nc, Ng), np.float32), np.ones((Nc, Ng), np.float32), Q.directions(np.arange(float(Nc))), np.ones(Nc)


def planted_genes(Ng=2, K=3, NW=1):
    z = np.zeros(Ng)
    return GeneJointFit(means=np.zeros((K, Ng)), log_gamma=z.copy(), log_beta=np.full(Ng, 2.0), cov=np.zeros((Ng, K + 2, K + 2)),
                        stds=np.ones((K + 2, Ng)), loglik_S=z, loglik_U=z, decrement=z, iterations=np.zeros(Ng, np.int32),
                        status=np.zeros(Ng, np.int32), n_clamped=np.zeros(Ng, np.int32), score_w=np.zeros((Ng, NW)), info_w=np.zeros((Ng, NW, NW)))


def planted_fit(Ng=2, Nhw=1, Nx=1, K=3):
    return JointVelocityMapFit(nu_omega=np.full((Nhw, Nx), 0.4), stds=np.full((Nhw, Nx), 0.04), cov=np.eye(Nhw * Nx), F=0.0, dec=0.0, rounds=1,
                               status="CONVERGED", n_excluded=0, included=np.ones(Ng, bool), genes=planted_genes(Ng, K, Nhw * Nx))


def test_host_refusals_of_the_bootstrap_worker():
    """Each is a ValueError (or NotImplementedError) although no device is there: decided before any device work."""
    S, U, xy, n = small()
    fit = planted_fit()
    boot = velocity_map_joint_bootstrap
    with pytest.raises(ValueError, match="dispersion"):
        boot(S, U, xy, n, noisemodel="NegativeBinomial", dispersion="mle", fit=fit)
    for bad in (0, 65536, 2.5, -1, True):
        with pytest.raises(ValueError, match="n_boot"):
            boot(S, U, xy, n, n_boot=bad, fit=fit)
    big = np.ones((2, 30000), np.float32)
    with pytest.raises(ValueError, match="1 GiB"):
        boot(big, big, Q.directions(np.arange(2.0)), np.ones(2), n_boot=1000)
    for bad in (np.full((3, 6), -1.0), np.full((3, 6), np.nan), np.full((3, 6), np.inf), np.ones((3, 5)), np.ones(6)):
        with pytest.raises(ValueError, match="weights"):
            boot(S, U, xy, n, weights=bad, fit=fit)
    with pytest.raises(NotImplementedError):
        boot(S, U, xy, n, noisemodel="Lognormal", fit=fit)
    with pytest.raises(ValueError, match="counts_U must be"):
        boot(S, U[:, :1], xy, n, fit=fit)
    for bad in (planted_fit(Ng=3), planted_fit(Nx=2), planted_fit(Nhw=3), planted_fit(K=5), "a fit"):
        with pytest.raises(ValueError, match="fit must be"):
            boot(S, U, xy, n, n_boot=4, fit=bad)
    with pytest.raises(ValueError, match="harmonics must be"):
        boot(S, U, xy, n, 3, fit=fit)
    with pytest.raises(ValueError, match="nuw_start"):
        boot(S, U, xy, n, nuw_start=[0.1, 0.2], fit=fit)
    with pytest.raises(ValueError, match="max_rounds"):
        boot(S, U, xy, n, max_rounds=-1, fit=fit)
    with pytest.raises(ValueError, match="tol_outer"):
        boot(S, U, xy, n, tol_outer=-1.0, fit=fit)
    with pytest.raises(ValueError, match="storage"):
        boot(S, U, xy, n, storage="f16", fit=fit)
    names = list(inspect.signature(boot).parameters)
    assert names[:10] == ["counts_S", "counts_U", "directions", "n_scounts", "harmonics", "harmonics_w", "condition_design", "a", "noisemodel",
                          "dispersion"]
    assert names[10:17] == ["n_boot", "seed", "weights", "fit", "warm_start", "keep_genes", "return_weights"]
    sig = inspect.signature(boot).parameters
    assert sig["n_boot"].default == 200 and sig["seed"].default == 0 and sig["warm_start"].default is True and sig["max_iter"].default == 40
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[10:])
    extra = set(inspect.signature(velocity_map_joint).parameters) - set(names)
    assert extra == {"start", "refused"}, extra                              # velocity_map_joint's run options are all taken


def test_host_refusals_of_gene_joint_weighted():
    S, U, xy, n = small()
    for bad in (np.ones(5), np.full(6, -1.0), np.full(6, np.nan), np.ones((2, 5)), np.ones((2, 2, 6)), None):
        with pytest.raises(ValueError, match="weights"):
            gene_joint_weighted(S, U, xy, n, bad, 0.4)
    with pytest.raises(ValueError, match="either omega"):
        gene_joint_weighted(S, U, xy, n, np.ones(6))
    with pytest.raises(ValueError, match="evaluate_only needs start"):
        gene_joint_weighted(S, U, xy, n, np.ones(6), 0.4, evaluate_only=True)
    with pytest.raises(ValueError, match="1 GiB"):
        big = np.ones((2, 30000), np.float32)
        gene_joint_weighted(big, big, Q.directions(np.arange(2.0)), np.ones(2), np.ones((1000, 2)), 0.4)
    with pytest.raises(ValueError, match="n_boot"):
        gene_joint_bootstrap(S, U, xy, n, 0.4, n_boot=0)
    with pytest.raises(ValueError, match="fit must be"):
        gene_joint_bootstrap(S, U, xy, n, 0.4, n_boot=2, fit=planted_genes(Ng=3))
    # the unweighted functions refuse weights exactly as before
    with pytest.raises(NotImplementedError, match="case weights"):
        check_arguments(S, U, xy, n, cell_weights=np.ones(6))
    names = list(inspect.signature(gene_joint_weighted).parameters)
    from velocycle_amd.gene_joint import gene_joint
    plain = [k for k in inspect.signature(gene_joint).parameters if k != "refused"]
    assert names[:5] == ["counts_S", "counts_U", "directions", "n_scounts", "cell_weights"] and [k for k in names if k != "cell_weights"] == plain


def test_summaries_are_shared_and_gene_stds_skip_excluded_replicates():
    rep = np.zeros((5, 1, 2))
    rep[:, 0, 0] = [0.4, 0.5, 0.6, 9.0, 0.5]
    rep[:, 0, 1] = [0.2, 0.25, 0.2, 9.0, 0.1]
    status = np.array(["CONVERGED", "CONVERGED", "CONVERGED", "STALLED", "CONVERGED"])
    fit = planted_fit(Nx=2)
    rng = np.random.default_rng(1)
    theta = rng.normal(size=(5, 2, 5))
    inc = np.ones((5, 2), bool)
    inc[1, 0] = False                                                        # replicate 1 left gene 0 out
    theta[1, 0] = np.nan
    bs = JointVelocityMapBootstrap(rep, status, np.arange(5), np.zeros(5, np.int64), np.zeros(5), np.zeros(5), fit=fit,
                                   theta_replicates=theta, gene_status=np.zeros((5, 2), np.int32), gene_included=inc)
    base = VelocityMapBootstrap(rep, status, np.arange(5), np.zeros(5, np.int64), np.zeros(5), np.zeros(5), fit=fit)
    assert isinstance(bs, VelocityMapBootstrap) and JointVelocityMapBootstrap.contrast is VelocityMapBootstrap.contrast
    assert JointVelocityMapBootstrap.interval is VelocityMapBootstrap.interval and "means" not in vars(JointVelocityMapBootstrap)
    keep = rep[[0, 1, 2, 4]]
    assert list(bs.ok) == [True, True, True, False, True] and bs.n_ok == 4
    assert np.array_equal(bs.means, base.means) and np.array_equal(bs.stds, base.stds) and np.array_equal(bs.cov, base.cov)
    assert np.allclose(bs.stds, keep.std(0, ddof=1)) and np.allclose(bs.bias, keep.mean(0) - 0.4)
    assert bs.laplace_stds is None and "laplace_stds" in JointVelocityMapBootstrap.__dataclass_fields__       # the worker fills it
    assert math.isclose(bs.contrast_std(0, 1), np.std(np.log(keep[:, 0, 0] / keep[:, 0, 1]), ddof=1))
    lo, hi = bs.contrast_interval(0, 1, 0.5)
    assert lo <= np.median(bs.contrast(0, 1)[bs.ok]) <= hi
    sd = bs.gene_stds()
    assert sd.shape == (5, 2)
    assert np.allclose(sd[:, 0], theta[[0, 2, 4], 0].std(0, ddof=1))         # without the stalled replicate 3 and the excluding replicate 1
    assert np.allclose(sd[:, 1], theta[[0, 1, 2, 4], 1].std(0, ddof=1))
    inc[[0, 2], 0] = False
    assert np.isnan(bs.gene_stds()[:, 0]).all() and np.isfinite(bs.gene_stds()[:, 1]).all()      # one replicate left: no deviation
    cyc = bs.to_cycle(["a", "b"])
    assert np.array_equal(cyc.means.values, fit.genes.means) and np.array_equal(cyc.stds.values, bs.gene_stds()[:3], equal_nan=True)
    assert np.array_equal(cyc.log_betas, fit.genes.log_beta)
    with pytest.raises(ValueError, match="keep_genes"):
        JointVelocityMapBootstrap(rep, status, np.arange(5), np.zeros(5, np.int64), np.zeros(5), np.zeros(5), fit=fit).gene_stds()
    gb = GeneJointBootstrap(theta[:, :, :], np.zeros((5, 2), np.int32), np.ones((5, 2), bool), fit=fit.genes)
    assert np.allclose(gb.gene_stds()[:, 1], theta[:, 1].std(0, ddof=1))
    import velocycle_amd
    from velocycle_amd import joint_bootstrap as JB
    assert {"velocity_map_joint_bootstrap", "JointVelocityMapBootstrap", "gene_joint_weighted", "gene_joint_bootstrap",
            "GeneJointBootstrap"} <= set(velocycle_amd.__all__)
    assert velocycle_amd.velocity_map_joint_bootstrap is velocity_map_joint_bootstrap
    assert "sampling variability" in JB.__doc__.lower() and "NOT" in JB.__doc__ and "prior of gamma" in JB.__doc__


def test_containers_pop_bootstrap_by_name(monkeypatch):
    from velocycle_amd import gene_joint as GJ
    from velocycle_amd import joint_bootstrap as JB
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import AngularSpeed, Cycle, Phases
    p = Q.cases()["shape_65_4_2_Poisson"]
    S, U, xy, n = p["S"].astype(np.float32), p["U"].astype(np.float32), Q.directions(p["phis"]), p["n"]
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(65)])
    ad = AnnDataLite(S, U, gene_names=[f"g{i}" for i in range(4)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    seen, boot_seen = {}, {}
    the_fit = planted_fit(Ng=4, Nx=2, K=5)

    def fake(counts_S, counts_U, directions, n_scounts, **kw):
        seen.update(kw)
        return the_fit

    class Replicates:
        def to_cycle(self, names):
            out = the_fit.genes.to_cycle(names)
            out.stds.iloc[:, :] = 7.0
            return out

    def fake_boot(counts_S, counts_U, directions, n_scounts, **kw):
        boot_seen.update(kw, counts_U=counts_U)
        return Replicates()
    monkeypatch.setattr(GJ, "velocity_map_joint", fake)
    monkeypatch.setattr(JB, "velocity_map_joint_bootstrap", fake_boot)
    D = np.zeros((2, 65))
    D[0, :30], D[1, 30:] = 1, 1
    prior = AngularSpeed.trivial_prior(["a", "b"], harmonics=0)
    out, fit = AngularSpeed.from_joint_mle(None, ph, ad, 0, D, "NegativeBinomial", 0.2, cycle_harmonics=2, prior=prior, return_fit=True,
                                           max_rounds=7, bootstrap=16, bootstrap_seed=5)
    assert "bootstrap" not in seen and "bootstrap_seed" not in seen and seen["max_rounds"] == 7
    assert boot_seen["n_boot"] == 16 and boot_seen["seed"] == 5 and boot_seen["fit"] is fit and boot_seen["max_rounds"] == 7
    assert boot_seen["nuw_prior"] is prior and boot_seen["noisemodel"] == "NegativeBinomial" and boot_seen["dispersion"] == 0.2
    assert boot_seen["harmonics"] == 2 and boot_seen["harmonics_w"] == 0 and boot_seen["condition_design"] is D and boot_seen["keep_genes"]
    assert np.array_equal(boot_seen["counts_U"], U) and isinstance(fit.bootstrap, Replicates) and "bootstrap" not in fit.__dataclass_fields__
    assert np.array_equal(out.means.values, fit.nu_omega) and np.array_equal(out.stds.values, fit.stds)          # the Laplace stds, untouched
    the_fit.bootstrap = None
    boot_seen.clear()
    out0, fit0 = AngularSpeed.from_joint_mle(None, ph, ad, 0, D, "NegativeBinomial", 0.2, cycle_harmonics=2, prior=prior, return_fit=True)
    assert fit0.bootstrap is None and not boot_seen and out0.stds.equals(out.stds) and out0.means.equals(out.means)
    for bad in (-1, 2.5, "4", True):
        with pytest.raises(ValueError, match="bootstrap must be"):
            AngularSpeed.from_joint_mle(None, ph, ad, 0, D, prior=prior, bootstrap=bad)
        with pytest.raises(ValueError, match="bootstrap must be"):
            Cycle.from_joint_mle(ph, ad, 0.4, 2, bootstrap=bad)
    seen.clear()
    for bad in (-1, 2.5, "4", True, None):                                   # refused before the full fit runs
        with pytest.raises(ValueError, match="bootstrap_seed must be"):
            AngularSpeed.from_joint_mle(None, ph, ad, 0, D, prior=prior, bootstrap=2, bootstrap_seed=bad)
        with pytest.raises(ValueError, match="bootstrap_seed must be"):
            Cycle.from_joint_mle(ph, ad, 0.4, 2, bootstrap=2, bootstrap_seed=bad)
    assert not seen
    # the Cycle: the stds are the replicates', the means and the kinetics the fit's
    gseen, gboot = {}, {}

    def fake_genes(counts_S, counts_U, directions, n_scounts, **kw):
        gseen.update(kw)
        return the_fit.genes

    def fake_gene_boot(counts_S, counts_U, directions, n_scounts, **kw):
        gboot.update(kw)
        return Replicates()
    monkeypatch.setattr(GJ, "gene_joint", fake_genes)
    monkeypatch.setattr(JB, "gene_joint_bootstrap", fake_gene_boot)
    plain = Cycle.from_joint_mle(ph, ad, 0.4, 2, max_iter=9)
    assert gseen == dict(harmonics=2, a=1, noisemodel="Poisson", dispersion=0.3, prior_means=None, prior_stds=None, omega=0.4, max_iter=9)
    assert not gboot and np.array_equal(plain.stds.values, the_fit.genes.stds[:5]) and the_fit.genes.bootstrap is None
    cyc, gfit = Cycle.from_joint_mle(ph, ad, 0.4, 2, max_iter=9, bootstrap=8, return_fit=True)
    assert gboot["n_boot"] == 8 and gboot["seed"] == 0 and gboot["fit"] is gfit and gboot["omega"] == 0.4 and gboot["max_iter"] == 9
    assert (cyc.stds.values == 7.0).all() and np.array_equal(cyc.means.values, plain.means.values)
    assert np.array_equal(cyc.log_gammas, plain.log_gammas) and isinstance(gfit.bootstrap, Replicates)
