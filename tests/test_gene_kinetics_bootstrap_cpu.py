"""CPU: the checker of the weighted kinetics fit (tests/gene_kinetics_boot_checker.py) against itself, the bootstrap estimator of the
speed ratio's standard error on the float32 restatement, the header and binding of vc_gene_kinetics_weighted, its refusals and its code
object, the host-side refusals of `velocity_map_bootstrap`, `gene_kinetics(cell_weights=)` and `velocity_map(cell_weights=)`, the
summaries of `VelocityMapBootstrap` and the container's plumbing."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gene_kinetics_boot_checker as KB
from tests import gene_kinetics_checker as Q
from tests.test_gene_kinetics_cpu import REFUSALS as PLAIN_REFUSALS
from velocycle_amd.gene_kinetics import VelocityMapFit, GeneKineticsFit, _row_constants, gene_kinetics, velocity_map
from velocycle_amd.gene_harmonics import _constants
from velocycle_amd.kinetics_bootstrap import VelocityMapBootstrap, velocity_map_bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the checker
def test_left_out_pairs_are_the_two_empty_rows():
    """189 pairs over Q.FIT_CASES + Q.SCORE_CASES; the two rows of shape_1_1_1_Poisson whose only cell drew weight 0 have no fit, and no
    other pair is left out.  Every reference ends CONVERGED, every restatement from both starts CONVERGED / ROUNDING, kink-free."""
    total = sum(len(row) for name in KB.PAIR_CASES for row in KB.solved(name))
    assert total == 189, total
    lost = KB.left_out()
    Wt = KB.weights("shape_1_1_1_Poisson")
    assert lost == {("shape_1_1_1_Poisson", b, 0) for b in range(KB.ROWS) if Wt[b, 0] == 0} and len(lost) == 2, lost
    for name in KB.PAIR_CASES:
        for b, row in enumerate(KB.solved(name)):
            for g, s in enumerate(row):
                if s is None:
                    continue
                f64, f32, f32w, _ = s
                assert f64["status"] == Q.CONVERGED and f32["status"] in Q.INTERIOR and f32w["status"] in Q.INTERIOR, (name, b, g)
                assert min(f64["minz"], f32["minz"], f32w["minz"]) >= Q.MIN_Z, (name, b, g)


def test_bars_are_finite():
    bars = KB.bars()
    print("bars:", bars)
    print("unweighted bars:", Q.bars())
    assert set(bars) == set(Q.bars()) and all(np.isfinite(v) and v > 0 for v in bars.values()), bars


def test_expansion_equals_the_written_out_weighted_formulas():
    """On integer weights the two references are the same fit: the optimum within 1e-9 standard errors, and at one point every figure
    (objective, gradient, both matrices through the step, rounding scales, clamped cells, score, information) to rounding."""
    p, Wt = Q.cases()[KB.UNIFORM_CASE], KB.weights(KB.UNIFORM_CASE)
    worst, clamped = 0.0, 0
    for b, w in enumerate(Wt):
        pe = KB.expand(p, w)
        for g in range(p["U"].shape[1]):
            k, B, logm, nu, r = Q.gene_inputs(p, g)
            f64 = KB.solved(KB.UNIFORM_CASE)[b][g][0]
            ws = KB.weighted_solve64(k, B, logm, nu, p["W"], p["nuw"], w, p["noisemodel"], r)
            assert ws["status"] == Q.CONVERGED
            worst = max(worst, Q.xy_distance(ws["x"], ws["y"], f64))
            assert abs(ws["L"] - f64["L"]) <= 1e-10 * f64["abs"] and np.allclose(ws["inv"], f64["inv"], rtol=1e-8, atol=0)
            ke, Be, le, nue, re_ = Q.gene_inputs(pe, g)
            for x, y in ((0.0, 2.0), (-2.0, 2.5)):                           # the second point clamps cells
                a = KB.weighted_point64(x, y, k, B, logm, nu, p["W"], p["nuw"], w, p["noisemodel"], r)
                e = Q.point64(x, y, ke, Be, le, nue, pe["W"], p["nuw"], p["noisemodel"], re_)
                assert a["observed"] == e["observed"]
                for key in ("L", "abs", "f", "G", "M", "score", "info", "dec"):
                    assert np.allclose(a[key], e[key], rtol=1e-9, atol=1e-9 * abs(e["abs"])), (b, g, key, a[key], e[key])
                # the two exceptions.  The rounding scales (wt wo)^2 + (wt res)^2 weigh a repeated cell wt^2 times, the expansion wt
                # times: equal where no weight exceeds 1, else larger by at most max wt.  n_clamped counts CELLS with w > 0, the
                # expansion their copies: equal where no weight exceeds 1
                assert (a["N"] >= e["N"] * (1 - 1e-12)).all() and (a["N"] <= w.max() * e["N"] * (1 + 1e-12)).all()
                one = np.minimum(w, 1.0)
                p1 = KB.expand(p, one)
                a1 = KB.weighted_point64(x, y, k, B, logm, nu, p["W"], p["nuw"], one, p["noisemodel"], r)
                e1 = Q.point64(x, y, *Q.gene_inputs(p1, g)[:4], p1["W"], p["nuw"], p["noisemodel"], re_)
                assert np.allclose(a1["N"], e1["N"], rtol=1e-9) and np.allclose(a1["score_unit"], e1["score_unit"], rtol=1e-9)
                assert a["n_clamped"] == a1["n_clamped"] == e1["n_clamped"] <= e["n_clamped"]
                clamped += a["n_clamped"]
    assert clamped > 0
    print("worst distance, standard errors:", worst)
    assert worst <= 1e-9
    for row in KB.solved_uniform():                                          # the non-integer table has a reference everywhere
        assert all(s["status"] == Q.CONVERGED and s["minz"] >= Q.MIN_Z for s in row)
    for row in KB.solved_nu_rows():
        assert all(s[0]["status"] == Q.CONVERGED and s[0]["minz"] >= Q.MIN_Z for s in row)
    # the default start of the weighted formulas is the expansion's
    k, B, logm, nu, r = Q.gene_inputs(p, 0)
    ke, Be, le, nue, _ = Q.gene_inputs(KB.expand(p, Wt[0]), 0)
    assert np.allclose(KB.weighted_start(k, B, logm, nu, p["W"], p["nuw"], Wt[0]), Q.start_xy(ke, Be, le, nue, KB.expand(p, Wt[0])["W"], p["nuw"]),
                       rtol=1e-13)


def test_outer_cases_as_stated():
    """Both outer cases under 2 rows, started at the full data's angular speed: every reference CONVERGED in 3-4 rounds, the
    restatement in 1-3, no gene excluded, min z >= 0.28 over the references' traces; the per-row-cycle case likewise."""
    for rows in [KB.outer_solved(name) for name in Q.OUTER_CASES] + [KB.outer_solved(KB.NU_ROWS_OUTER, True)]:
        assert len(rows) == KB.OUTER_ROWS
        for m64, m32, trace in rows:
            print(m64["status"], m64["rounds"], m32["status"], m32["rounds"], min(z for _, z in trace))
            assert m64["status"] == m32["status"] == "CONVERGED" and 3 <= m64["rounds"] <= 4 and 1 <= m32["rounds"] <= 3
            assert m64["n_excluded"] == m32["n_excluded"] == 0 and min(z for _, z in trace) >= KB.OUTER_MIN_Z


def _log_ratio_se(m):
    v, c = m["nuw"], m["cov"]
    return math.sqrt(c[0, 0] / v[0] ** 2 + c[1, 1] / v[1] ** 2 - 2 * c[0, 1] / (v[0] * v[1]))


def test_the_bootstrap_sees_what_the_laplace_error_of_a_poisson_fit_misses():
    """Negative-binomial counts (r = 3), two conditions: simulate(41, 1500, 30, 1, NB, [0.45, 0.3], Nx=2, level=(4.0, 5.5)).  40 Poisson(1)
    resamples from default_rng(12), each replicate the restatement's outer fit (map32) of the cell-expanded data started at the full
    fit.  Fitted as Poisson the bootstrap standard error of ln(omega_0 / omega_1) exceeds the Laplace one by at least 1.5 x (measured
    with 60 replicates: 0.0655 against 0.0221, 2.96 x); fitted as negative binomial the two agree within [0.6, 1.6] (0.0500 against
    0.0549, 0.91)."""
    p = Q.simulate(41, 1500, 30, 1, Q.NB, [0.45, 0.3], Nx=2, level=(4.0, 5.5))
    Wt = np.random.default_rng(12).poisson(1, (60, 1500))[:40]
    ratio = {}
    for noise, prob in ((Q.NB, p), (Q.PO, dict(p, noisemodel=Q.PO, r=None))):
        full = Q.map32(prob)
        assert full["status"] == "CONVERGED"
        reps = []
        for w in Wt:
            m = Q.map32(KB.expand(prob, w), nuw0=full["nuw"])
            assert m["status"] == "CONVERGED"
            reps.append(math.log(m["nuw"][0] / m["nuw"][1]))
        ratio[noise] = (np.std(reps, ddof=1), _log_ratio_se(full))
        print(f"{noise}: bootstrap se {ratio[noise][0]:.4f}, Laplace se {ratio[noise][1]:.4f}, ratio {ratio[noise][0] / ratio[noise][1]:.2f}")
    assert ratio[Q.PO][0] >= 1.5 * ratio[Q.PO][1], ratio
    assert 0.6 <= ratio[Q.NB][0] / ratio[Q.NB][1] <= 1.6, ratio


# ---------------------------------------------------------------------------------------------------------------- the C side
def test_header_declares_and_lib_binds_vc_gene_kinetics_weighted():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert " *   vc_gene_kinetics_weighted " in hdr and "#define VC_ABI_VERSION 2" in hdr
    decl = re.search(r"\bint vc_gene_kinetics_weighted\(([^;]*)\);", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert len(_lib.EXPORTS["vc_gene_kinetics_weighted"][1]) == len(names) == 34 and names[-1] == "hip_stream"
    plain = [a.split()[-1].lstrip("*") for a in re.search(r"\bint vc_gene_kinetics\(([^;]*)\);", hdr).group(1).split(",")]
    added = ["nu_row_stride", "nuw_row_stride", "weights_dev", "R", "weight_stride", "start_row_stride"]
    assert [n for n in names if n not in added] == plain and [n for n in names if n in added] == added
    types = _lib.EXPORTS["vc_gene_kinetics_weighted"][1]
    assert all(types[names.index(n)] is (C.c_void_p if n == "weights_dev" else C.c_int64) for n in added)
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_kinetics_weighted.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace {")[1]
    assert f"KINW_BOUND = {Q.BOUND};" in src and f"KINW_MAX_HALVINGS = {Q.HALVINGS};" in src and "KINW_FLOOR = 1.0e-5;" in src
    assert "KINW_SLAB = 65535;" in src and "KINW_MAX_ROWS = 65535;" in src


def kinw_args(**k):
    """Arguments of vc_gene_kinetics_weighted with pointers that are never dereferenced: every call made with them is refused before
    the launch."""
    one = C.c_void_p(64)
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("nu", one), k.get("nu_stride", 0), k.get("w", one), k.get("NW", 1), k.get("nuw", one),
            k.get("nuw_stride", 0), k.get("noise", 1), k.get("r", None), k.get("prior", one), k.get("weights", one), k.get("R", 2),
            k.get("wstride", 4), k.get("start", None), k.get("start_stride", 0), k.get("tol", 1e-10), k.get("max_iter", 25),
            k.get("xy", one), k.get("cov", one), k.get("ll", one), k.get("dec", one), k.get("it", one), k.get("st", one), k.get("nc", one),
            k.get("score", one), k.get("info", one), None]


# vc_gene_kinetics' refusals (cov_dev may be NULL here), then the weighted entry point's own
REFUSALS = [(kw, msg) for kw, msg in PLAIN_REFUSALS if kw != dict(cov=None)] + \
    [(dict(weights=None), b"null weights_dev"), (dict(R=0), b"R must be"), (dict(R=65536), b"R must be"), (dict(wstride=3), b"weight_stride"),
     (dict(nu_stride=11), b"nu_row_stride"), (dict(nu_stride=-12), b"nu_row_stride"), (dict(nuw_stride=2, NW=3), b"nuw_row_stride"),
     (dict(start=C.c_void_p(64), start_stride=7), b"start_row_stride"), (dict(start=C.c_void_p(64), start_stride=-8), b"start_row_stride")]
# the order: a shared refusal wins over an own one, vc_gene_kinetics' over the weights'
ORDER = [(dict(K=2, weights=None), b"K must be"), (dict(counts=None, weights=None), b"null input"), (dict(weights=None, R=0), b"null weights_dev"),
         (dict(R=0, wstride=3), b"R must be"), (dict(wstride=3, nu_stride=1), b"weight_stride"), (dict(max_iter=0, weights=None), b"start_dev")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert len(REFUSALS) == len(PLAIN_REFUSALS) - 1 + 9
    for kw, msg in REFUSALS + ORDER:
        assert lib.vc_gene_kinetics_weighted(*kinw_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), (kw, lib.vc_last_error(None))
        assert lib.vc_last_error(None).startswith(b"vc_gene_kinetics_weighted: ")
    assert lib.vc_gene_kinetics_weighted(*kinw_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    # the shared refusals and every refusal of its own come before the launch
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_kinetics_weighted.hip")).read()
    body = src[src.index('extern "C" int vc_gene_kinetics_weighted('):]
    launch = body.index("hipLaunchKernelGGL")
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < launch
    assert body.rindex("gene_fail(") < launch < body.index("gene_launched(")


def test_the_code_object(tmp_path):
    """All 32 instantiations of vc_gene_kinetics_weighted_kernel (H {1, 2} x NW 0..3 x {NB, Poisson} x {u16, f32}) in the assembly
    emitted for gfx950: .private_segment_fixed_size 0 (no scratch), at most 256 VGPRs, at most 1024 bytes of LDS."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_kinetics_weighted.hip")
    out = str(tmp_path / "kinw.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*vc_gene_kinetics_weighted_kernel\S*)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(found) == 32 and len({name for _, name, _, _ in found}) == 32, len(found)
    print("VGPRs:", sorted({int(v) for _, _, _, v in found}), "LDS:", sorted({int(lds) for lds, _, _, _ in found}))
    assert all(int(p) == 0 for _, _, p, _ in found), found
    assert all(int(lds) <= 1024 and int(v) <= 256 for lds, _, _, v in found), found


# ---------------------------------------------------------------------------------------------------------------- the Python side
def small(Nc=6, Ng=2):
    return np.ones((Nc, Ng), np.float32), Q.directions(np.arange(float(Nc))), np.ones(Nc), np.zeros((3, Ng))


def planted_fit(Ng=2, Nhw=1, Nx=1):
    kin = GeneKineticsFit(np.zeros(Ng), np.full(Ng, 2.0), *[None] * 9)
    return VelocityMapFit(nu_omega=np.full((Nhw, Nx), 0.4), stds=np.full((Nhw, Nx), 0.04), cov=np.eye(Nhw * Nx), F=0.0, dec=0.0, rounds=1,
                          status="CONVERGED", n_excluded=0, included=np.ones(Ng, bool), kinetics=kin)


def test_host_refusals_of_the_bootstrap_worker():
    """Each is a ValueError (or NotImplementedError) although no device is there: decided before any device work."""
    U, xy, n, nu = small()
    fit = planted_fit()
    with pytest.raises(ValueError, match="dispersion"):
        velocity_map_bootstrap(U, xy, n, nu, noisemodel="NegativeBinomial", dispersion="mle", fit=fit)
    for bad in (0, 65536, 2.5, -1):
        with pytest.raises(ValueError, match="n_boot"):
            velocity_map_bootstrap(U, xy, n, nu, n_boot=bad, fit=fit)
    with pytest.raises(ValueError, match="1 GiB"):
        velocity_map_bootstrap(np.ones((2, 30000), np.float32), Q.directions(np.arange(2.0)), np.ones(2), np.zeros((3, 30000)), n_boot=1000)
    for bad in (np.full((3, 6), -1.0), np.full((3, 6), np.nan), np.full((3, 6), np.inf), np.ones((3, 5)), np.ones(6)):
        with pytest.raises(ValueError, match="weights"):
            velocity_map_bootstrap(U, xy, n, nu, weights=bad, fit=fit)
    with pytest.raises(NotImplementedError):
        velocity_map_bootstrap(U, xy, n, nu, noisemodel="Lognormal", fit=fit)
    for rep in (np.zeros((3, 3, 2)), np.zeros((4, 5, 2)), np.zeros((4, 3, 3))):
        with pytest.raises(ValueError, match="means_replicates"):
            velocity_map_bootstrap(U, xy, n, nu, n_boot=4, means_replicates=rep, fit=fit)
    with pytest.raises(ValueError, match="means_replicates"):
        velocity_map_bootstrap(U, xy, n, nu, weights=np.ones((2, 6)), means_replicates=np.zeros((3, 3, 2)), fit=fit)
    for bad in (planted_fit(Ng=3), planted_fit(Nx=2), planted_fit(Nhw=3)):
        with pytest.raises(ValueError, match="fit must be"):
            velocity_map_bootstrap(U, xy, n, nu, n_boot=4, fit=bad)
    with pytest.raises(ValueError, match="means must be"):
        velocity_map_bootstrap(U, xy, n, np.zeros((7, 2)), fit=fit)
    with pytest.raises(ValueError, match="nuw_start"):
        velocity_map_bootstrap(U, xy, n, nu, nuw_start=[0.1, 0.2], fit=fit)
    with pytest.raises(ValueError, match="max_rounds"):
        velocity_map_bootstrap(U, xy, n, nu, max_rounds=-1, fit=fit)
    with pytest.raises(ValueError, match="storage"):
        velocity_map_bootstrap(U, xy, n, nu, storage="f16", fit=fit)
    names = list(inspect.signature(velocity_map_bootstrap).parameters)
    assert names[:9] == ["counts_U", "directions", "n_scounts", "means", "harmonics_w", "condition_design", "a", "noisemodel", "dispersion"]
    assert names[9:18] == ["n_boot", "seed", "weights", "fit", "means_replicates", "warm_start", "keep_kinetics", "return_weights", "prior"]
    sig = inspect.signature(velocity_map_bootstrap).parameters
    assert sig["n_boot"].default == 200 and sig["seed"].default == 0 and sig["warm_start"].default is True
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names[9:])
    extra = set(inspect.signature(velocity_map).parameters) - set(names)
    assert extra == {"cell_weights"}, extra                                 # velocity_map's run options are all taken


def test_host_refusals_of_cell_weights():
    U, xy, n, nu = small()
    for bad in (np.ones(5), np.full(6, -1.0), np.full(6, np.nan), np.ones((2, 5)), np.ones((2, 2, 6))):
        with pytest.raises(ValueError, match="weights"):
            gene_kinetics(U, xy, n, nu, 0.4, cell_weights=bad)
    for bad in (np.ones(5), np.full(6, -1.0), np.full(6, np.inf), np.ones((2, 6)), np.ones((1, 6))):
        with pytest.raises(ValueError, match="weights"):
            velocity_map(U, xy, n, nu, cell_weights=bad)
    with pytest.raises(ValueError, match="means_replicates needs cell_weights"):
        gene_kinetics(U, xy, n, nu, 0.4, means_replicates=np.zeros((2, 3, 2)))
    with pytest.raises(ValueError, match="means_replicates must be"):
        gene_kinetics(U, xy, n, nu, 0.4, cell_weights=np.ones((2, 6)), means_replicates=np.zeros((3, 3, 2)))
    assert inspect.signature(gene_kinetics).parameters["cell_weights"].default is None
    assert inspect.signature(velocity_map).parameters["cell_weights"].default is None


def test_row_constants_are_constants_row_by_row():
    """The [R, n] constants of the weighted log-likelihood are `_constants(blk, r64, w64)` of each row bit for bit, and a row of ones
    is the unweighted constant bit for bit."""
    rng = np.random.default_rng(3)
    blk = torch.from_numpy(rng.poisson(3.0, (5, 37)).astype(np.float32))
    W64 = torch.from_numpy(np.concatenate([rng.poisson(1, (2, 37)).astype(np.float64), np.ones((1, 37))]))
    for r64 in (None, torch.from_numpy(rng.uniform(1, 5, 5))):
        got = _row_constants(blk, r64, W64)
        for b in range(3):
            assert got[b].numpy().tobytes() == _constants(blk, r64, W64[b]).numpy().tobytes()
        assert got[2].numpy().tobytes() == _constants(blk, r64).numpy().tobytes()


def test_summaries_and_contrast_on_planted_replicates():
    rep = np.zeros((5, 1, 2))
    rep[:, 0, 0] = [0.4, 0.5, 0.6, 9.0, 0.5]
    rep[:, 0, 1] = [0.2, 0.25, 0.2, 9.0, -0.1]
    status = np.array(["CONVERGED", "CONVERGED", "CONVERGED", "STALLED", "CONVERGED"])
    fit = planted_fit(Nx=2)
    bs = VelocityMapBootstrap(rep, status, np.arange(5), np.zeros(5, np.int64), np.zeros(5), np.zeros(5), fit=fit)
    keep = rep[[0, 1, 2, 4]]
    assert list(bs.ok) == [True, True, True, False, True] and bs.n_ok == 4
    assert np.allclose(bs.means, keep.mean(0)) and bs.means.shape == (1, 2)
    assert np.allclose(bs.stds, keep.std(0, ddof=1)) and np.allclose(bs.cov, np.cov(keep[:, 0, :].T, ddof=1))
    assert np.allclose(bs.bias, keep.mean(0) - 0.4)
    lo, hi = bs.interval(0.5)
    assert np.allclose(lo, np.quantile(keep, 0.25, axis=0)) and np.allclose(hi, np.quantile(keep, 0.75, axis=0))
    c = bs.contrast(0, 1)
    assert c.shape == (5,) and np.allclose(c[:4], np.log(rep[:4, 0, 0] / rep[:4, 0, 1])) and np.isnan(c[4])       # a speed <= 0: no logarithm
    assert np.allclose(bs.contrast(1, 0)[:3], -c[:3]) and np.allclose(bs.contrast(0, 1, log=False), rep[:, 0, 0] - rep[:, 0, 1])
    assert np.isnan(bs.contrast_std(0, 1))                                   # a NaN among the ok replicates shows
    assert math.isclose(bs.contrast_std(0, 1, log=False), np.std((rep[:, 0, 0] - rep[:, 0, 1])[[0, 1, 2, 4]], ddof=1))
    dlo, dhi = bs.contrast_interval(0, 1, 0.5, log=False)
    assert math.isclose(dlo, np.quantile((rep[:, 0, 0] - rep[:, 0, 1])[[0, 1, 2, 4]], 0.25)) and dlo <= dhi
    three = VelocityMapBootstrap(rep[:3], status[:3], np.arange(3), np.zeros(3, np.int64), np.zeros(3), np.zeros(3), fit=fit)
    assert math.isclose(three.contrast_std(0, 1), np.std(np.log(rep[:3, 0, 0] / rep[:3, 0, 1]), ddof=1))
    l3, h3 = three.contrast_interval(0, 1, 0.9)
    assert l3 <= np.median(three.contrast(0, 1)) <= h3
    for bad in ((0, 2), (-1, 0), (0.5, 1)):
        with pytest.raises(ValueError):
            bs.contrast(*bad)
    with pytest.raises(ValueError):
        bs.interval(1.0)
    # condition-major covariance with harmonics: [R, 3, 2] -> 6 x 6, stds back in the row layout
    rng = np.random.default_rng(0)
    big = VelocityMapBootstrap(rng.normal(size=(7, 3, 2)), np.array(["CONVERGED"] * 7), np.arange(7), np.zeros(7, np.int64), np.zeros(7), np.zeros(7))
    flat = big.nu_omega_replicates.transpose(0, 2, 1).reshape(7, 6)
    assert np.allclose(big.cov, np.cov(flat.T, ddof=1)) and np.allclose(big.stds, big.nu_omega_replicates.std(0, ddof=1))
    none = VelocityMapBootstrap(rep, np.array(["STALLED"] * 5), np.arange(5), np.zeros(5, np.int64), np.zeros(5), np.zeros(5), fit=fit)
    assert none.n_ok == 0 and np.isnan(none.means).all() and np.isnan(none.stds).all() and np.isnan(none.contrast_std(0, 1))
    assert "sampling variability" in VelocityMapBootstrap.__doc__.lower() and "not replace" in VelocityMapBootstrap.__doc__
    import velocycle_amd
    assert {"velocity_map_bootstrap", "VelocityMapBootstrap"} <= set(velocycle_amd.__all__)
    assert velocycle_amd.velocity_map_bootstrap is velocity_map_bootstrap


def test_container_pops_bootstrap_by_name(monkeypatch):
    from velocycle_amd import gene_kinetics as GK
    from velocycle_amd import kinetics_bootstrap as KBS
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import AngularSpeed, Cycle, Phases
    p = Q.cases()["shape_65_4_2_Poisson"]
    U, xy, n, means = p["U"].astype(np.float32), Q.directions(p["phis"]), p["n"], p["nu"].T
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(65)])
    ad = AnnDataLite(U * 2, U, gene_names=[f"g{i}" for i in range(4)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    cyc = Cycle.from_array(means, np.ones_like(means), gene_names=list(ad.var.index))
    seen, boot_seen = {}, {}

    def fake(counts, directions, n_scounts, means_, **kw):
        seen.update(kw)
        return planted_fit(Ng=4, Nx=2)

    def fake_boot(counts, directions, n_scounts, means_, **kw):
        boot_seen.update(kw, counts=counts)
        return "the replicates"
    monkeypatch.setattr(GK, "velocity_map", fake)
    monkeypatch.setattr(KBS, "velocity_map_bootstrap", fake_boot)
    D = np.zeros((2, 65))
    D[0, :30], D[1, 30:] = 1, 1
    prior = AngularSpeed.trivial_prior(["a", "b"], harmonics=0)
    out, fit = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, D, "NegativeBinomial", 0.2, prior=prior, return_fit=True, max_rounds=7,
                                              bootstrap=16, bootstrap_seed=5)
    assert "bootstrap" not in seen and "bootstrap_seed" not in seen and seen["max_rounds"] == 7
    assert boot_seen["n_boot"] == 16 and boot_seen["seed"] == 5 and boot_seen["fit"] is fit and boot_seen["max_rounds"] == 7
    assert boot_seen["nuw_prior"] is prior and boot_seen["noisemodel"] == "NegativeBinomial" and boot_seen["dispersion"] == 0.2
    assert boot_seen["harmonics_w"] == 0 and boot_seen["condition_design"] is D and np.array_equal(boot_seen["counts"], U)
    assert fit.bootstrap == "the replicates" and "bootstrap" not in fit.__dataclass_fields__
    assert np.array_equal(out.means.values, fit.nu_omega) and np.array_equal(out.stds.values, fit.stds)          # the Laplace stds, untouched
    boot_seen.clear()
    out0, fit0 = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, D, "NegativeBinomial", 0.2, prior=prior, return_fit=True)
    assert fit0.bootstrap is None and not boot_seen and out0.stds.equals(out.stds)
    alone = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, D, "NegativeBinomial", 0.2, prior=prior, bootstrap=3)
    assert alone.stds.equals(out.stds) and boot_seen["n_boot"] == 3 and boot_seen["seed"] == 0
    for bad in (-1, 2.5, "4", True):
        with pytest.raises(ValueError, match="bootstrap must be"):
            AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, D, prior=prior, bootstrap=bad)
