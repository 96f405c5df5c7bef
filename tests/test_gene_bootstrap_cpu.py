"""CPU: the checker of the weighted per-gene fit (tests/gene_boot_checker.py) against itself, the bootstrap estimator on the float64
reference, the host-side refusals of `gene_harmonics_bootstrap` and `gene_harmonics(cell_weights=)`, the summaries of
`GeneHarmonicBootstrap`, the C entry point's refusals and the kernel's code object (no scratch)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gene_boot_checker as W
from tests import gene_glm_checker as G
from velocycle_amd.gene_bootstrap import GeneHarmonicBootstrap, gene_harmonics_bootstrap
from velocycle_amd.gene_harmonics import gene_harmonics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_left_out_share():
    """At most 10 % of the pairs of a case separate under their resample, none in a case with Nc >= 255; with this seed 3 of 35 in
    (65, 7, 3) for either noise and no other."""
    lost = {}
    for name, (p, w) in W.cases().items():
        keep = W.bearing(name)
        lost[name] = int((~keep).sum())
        assert lost[name] <= 0.1 * keep.size, (name, lost[name], keep.size)
        if p["S"].shape[0] >= 255:
            assert lost[name] == 0, (name, lost[name])
    assert {n: v for n, v in lost.items() if v} == {"shape_65_7_3_Poisson": 3, "shape_65_7_3_NegativeBinomial": 3}, lost


def test_bars_are_finite_and_capped():
    bars = W.bars()
    print("bars:", bars)
    assert all(np.isfinite(v) and v > 0 for v in bars.values()), bars
    assert bars["coef"] <= G.COEF_CAP, bars


def test_expansion_equals_the_written_out_weighted_newton():
    """On integer weights the two references are the same fit: within 1e-10 standard errors, and the same log-likelihood, on every
    integer-weight case."""
    worst = 0.0
    for name, (p, Wt) in W.cases().items():
        if not W.is_integer(name):
            continue
        keep = W.bearing(name)
        for b, w in enumerate(Wt):
            for g in range(p["S"].shape[1]):
                if not keep[b, g]:
                    continue
                k, B, logm, r, prior = G._gene_inputs(p, g)
                f64 = W.solved(name)[b][g][0]
                wn = W.weighted_newton64(k, B, logm, w, p["noisemodel"], r, prior)
                assert wn["status"] == G.CONVERGED
                d = wn["nu"] - f64["nu"]
                worst = max(worst, float(np.sqrt(max(d @ f64["hess"] @ d, 0.0))))
                assert abs(wn["loglik"] - f64["loglik"]) <= 1e-10 * f64["abs"], (name, b, g)
                assert np.allclose(wn["hess"], f64["hess"], rtol=1e-9, atol=0)
    print("worst distance, standard errors:", worst)
    assert worst <= 1e-10


def test_the_bootstrap_repairs_the_hessian_stds_of_a_misspecified_fit():
    """simulated(3000, 8), gene 4, H = 1, 200 Poisson(1) resamples, float64 reference only.  At the gene's true dispersion bootstrap and
    Hessian agree within 6 standard errors of a standard deviation estimated from 200 draws (relative standard error 1 / sqrt(2 * 199));
    for the Poisson fit of the same overdispersed counts the bootstrap is at least 1.15 x wider on every coefficient."""
    sim = G.simulated(3000, 8)
    g = G.PERMUTED_GENE
    k, B, logm = np.trunc(sim["S"][:, g]), G.basis64(sim["phis"], 1), np.log(sim["n"])
    Wt = np.random.default_rng(7).poisson(1, (200, 3000))
    ratios = {}
    for noise, r in (("NegativeBinomial", 1.0 / float(sim["shape_inv"][g])), ("Poisson", None)):
        full = G.newton64(k, B, logm, noise, r)
        assert full["status"] == G.CONVERGED
        reps = []
        for w in Wt:
            f = G.newton64(*W.expand(k, B, logm, w), noise, r)
            assert f["status"] == G.CONVERGED
            reps.append(f["nu"])
        ratios[noise] = np.std(np.array(reps), axis=0, ddof=1) / full["std"]
    print("std_boot / std_hess:", ratios)
    assert (np.abs(ratios["NegativeBinomial"] - 1) <= 6 / math.sqrt(2 * 199)).all(), ratios
    assert (ratios["Poisson"] >= 1.15).all(), ratios


def _inputs(Nc=6, Ng=2):
    return np.ones((Nc, Ng), np.float32), G.directions(np.arange(float(Nc))), np.ones(Nc)


def test_host_refusals_of_the_bootstrap_worker():
    S, xy, n = _inputs()
    with pytest.raises(ValueError, match="mle"):
        gene_harmonics_bootstrap(S, xy, n, noisemodel="NegativeBinomial", dispersion="mle")
    for bad in (0, 65536, 2.5):
        with pytest.raises(ValueError, match="n_boot"):
            gene_harmonics_bootstrap(S, xy, n, n_boot=bad)
    with pytest.raises(ValueError, match="1 GiB"):
        gene_harmonics_bootstrap(np.ones((2, 30000), np.float32), G.directions(np.arange(2.0)), np.ones(2), harmonics=3, n_boot=1000)
    for bad in (np.full((3, 6), -1.0), np.full((3, 6), np.nan), np.full((3, 6), np.inf), np.ones((3, 5)), np.ones(6)):
        with pytest.raises(ValueError, match="weights"):
            gene_harmonics_bootstrap(S, xy, n, weights=bad)
    with pytest.raises(NotImplementedError):
        gene_harmonics_bootstrap(S, xy, n, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="fit.means"):
        gene_harmonics_bootstrap(S, xy, n, fit=type("F", (), {"means": np.zeros((5, 2))})())


def test_host_refusals_of_cell_weights():
    S, xy, n = _inputs()
    with pytest.raises(ValueError, match="mle"):
        gene_harmonics(S, xy, n, noisemodel="NegativeBinomial", dispersion="mle", cell_weights=np.ones(6))
    for bad in (np.ones(5), np.ones((1, 6)), np.full(6, -1.0), np.full(6, np.nan)):
        with pytest.raises(ValueError, match="weights"):
            gene_harmonics(S, xy, n, cell_weights=bad)


def test_summaries_on_a_hand_made_replicate_array():
    # 4 replicates, H = 1, 3 genes: gene 0 all ok, gene 1 one ok, gene 2 none
    rep = np.zeros((4, 3, 3))
    rep[:, 0, 0] = [1.0, 2.0, 3.0, 100.0]
    rep[:, 1, 0] = [0.0, 1.0, 0.0, -1.0]                          # sin
    rep[:, 2, 0] = [1.0, 0.0, -1.0, 0.0]                          # cos
    rep[:, :, 1] = [[5.0, 3.0, 4.0], [np.nan] * 3, [-np.inf, 0, 0], [7.0, 7.0, 7.0]]
    rep[:, :, 2] = np.nan
    status = np.array([[0, 0, 2], [1, 3, 2], [0, 2, 4], [4, 4, 3]], dtype=np.int32)
    fit = type("F", (), {"means": np.ones((3, 3))})()
    bs = GeneHarmonicBootstrap(rep, status, np.zeros((4, 3), np.int32), fit=fit)
    assert bs.harmonics == 1
    assert np.array_equal(bs.ok, np.array([[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=bool))
    assert list(bs.n_ok) == [3, 1, 0]
    assert np.allclose(bs.means[:, 0], [2.0, 1 / 3, 0.0]) and np.array_equal(bs.means[:, 1], [5.0, 3.0, 4.0]) and np.isnan(bs.means[:, 2]).all()
    assert np.allclose(bs.stds[:, 0], np.std(rep[:3, :, 0], axis=0, ddof=1))          # ddof 1 over the ok replicates only
    assert np.isnan(bs.stds[:, 1]).all() and np.isnan(bs.stds[:, 2]).all()          # below 2 ok replicates
    assert np.allclose(bs.cov[0], np.cov(rep[:3, :, 0].T, ddof=1)) and np.isnan(bs.cov[1]).all()
    assert np.allclose(bs.bias[:, 0], bs.means[:, 0] - 1.0)
    assert np.allclose(bs.quantile(0.5)[:, 0], [2.0, 0.0, 0.0]) and np.array_equal(bs.quantile(0.5)[:, 1], [5.0, 3.0, 4.0])
    assert np.isnan(bs.quantile(0.5)[:, 2]).all()
    assert np.allclose(bs.amplitude(1)[:, 0], 1.0) and bs.amplitude(1)[0, 1] == 5.0
    assert np.allclose(bs.peak_phase(1)[:, 0], [0.0, np.pi / 2, np.pi, -np.pi / 2])
    lo, hi = bs.interval(0.5)
    assert np.allclose(lo[:, 0], np.quantile(rep[:3, :, 0], 0.25, axis=0)) and np.allclose(hi[:, 0], np.quantile(rep[:3, :, 0], 0.75, axis=0))
    alo, ahi = bs.interval(0.9, amplitude=1)
    assert np.allclose([alo[0], ahi[0]], 1.0) and alo[1] == ahi[1] == 5.0 and np.isnan(alo[2])
    # peaks at 0, pi / 2, pi over the ok replicates: the mean resultant is (0, 1) / 3
    assert np.allclose(bs.peak_phase_std(1)[0], math.sqrt(-2 * math.log(1 / 3))) and np.isnan(bs.peak_phase_std(1)[1:]).all()
    with pytest.raises(ValueError):
        bs.amplitude(2)


def boot_args(**k):
    """Arguments of vc_gene_glm_weighted with pointers that are never dereferenced: every call made with them is refused before the
    launch."""
    one = C.c_void_p(64)
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("noise", 1), k.get("r", None), k.get("pm", None), k.get("pp", None), k.get("weights", one),
            k.get("R", 2), k.get("wstride", 4), k.get("start", None), k.get("tol", 1e-10), k.get("max_iter", 25), k.get("nu", one),
            k.get("cov", None), k.get("ll", one), k.get("dec", one), k.get("it", one), k.get("st", one), None]


REFUSALS = [(dict(K=2), b"K must be"), (dict(counts=None), b"null input"), (dict(nu=None), b"null output"), (dict(st=None), b"null output"),
            (dict(Nc=0), b"Ng and Nc"), (dict(stride=3), b"gene_stride"), (dict(max_iter=0), b"max_iter"), (dict(tol=-1.0), b"tol"),
            (dict(noise=0), b"r_dev"), (dict(pm=C.c_void_p(64)), b"prior"),
            (dict(weights=None), b"null weights_dev"), (dict(R=0), b"R must be"), (dict(R=65536), b"R must be"),
            (dict(wstride=3), b"weight_stride")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.vc_gene_glm_weighted(*boot_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    for kw, msg in REFUSALS:
        assert lib.vc_gene_glm_weighted(*boot_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
        assert lib.vc_last_error(None).startswith(b"vc_gene_glm_weighted: ")
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_glm_weighted.hip")).read()
    body = src[src.index('extern "C" int vc_gene_glm_weighted'):]
    launch = body.index("hipLaunchKernelGGL")                                            # every refusal comes before the launch
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < body.rindex("gene_fail(") < launch
    header = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert "int vc_gene_glm_weighted(" in header and "#define VC_ABI_VERSION 2" in header


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_gene_glm_weighted_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly emitted
    for gfx950 (hipcc -S --cuda-device-only)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_glm_weighted.hip")
    out = str(tmp_path / "glmw.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    found = re.findall(r"\.name:\s+(\S*vc_gene_glm_weighted_kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read())
    assert len(found) == 16, len(found)                    # H 0..3 x {Poisson, NB} x {u16, f32}
    assert all(int(p) == 0 for _, p in found), found
