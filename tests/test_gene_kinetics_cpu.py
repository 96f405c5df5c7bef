"""CPU: the checker of the kinetics fit (tests/gene_kinetics_checker.py) against finite differences and the simulation's truth; the
fixtures' kink properties; the public face of `gene_kinetics` / `velocity_map` / `AngularSpeed.from_kinetics_mle` (refusals before any
device work, container plumbing); the C ABI declaration, its binding and its refusals; the kernel's code object.  Every test prints the
figures it asserts on."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gene_kinetics_checker as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_d_is_the_derivative_basis_applied_to_nu():
    """d from the basis rows themselves = nu . torch_fourier_basis(der=1), restated locally; and the product's own function agrees."""
    from velocycle_amd.utils import torch_fourier_basis
    rng = np.random.default_rng(0)
    phis = rng.uniform(0, 2 * np.pi, 300)
    for H in (1, 2):
        nu = rng.normal(size=2 * H + 1)
        want = nu @ Q.dbasis64(phis, H)
        got = Q.d_from_basis(nu, Q.basis64(phis, H))
        ours = torch_fourier_basis(torch.tensor(phis), H, der=1).double().numpy().T
        h = 1e-6
        fd = nu @ (Q.basis64(phis + h, H) - Q.basis64(phis - h, H)) / (2 * h)
        print(f"H = {H}: |d - nu . dB| {np.abs(got - want).max():.3g}, against the central difference {np.abs(got - fd).max():.3g}")
        assert np.abs(got - want).max() <= 8 * Q.EPS64 * np.abs(nu).sum() * H
        assert np.abs(got - fd).max() <= 1e-8 and np.abs(Q.dbasis64(phis, H).T - ours.T).max() <= 4 * Q.EPS32 * H


def test_gradient_and_observed_matrix_are_the_derivatives_of_f():
    p = Q.cases()["shape_257_5_1_NegativeBinomial"]
    for g in (0, 3):
        k, B, logm, nu, r = Q.gene_inputs(p, g)
        f = lambda x, y: Q.point64(x, y, k, B, logm, nu, p["W"], p["nuw"], p["noisemodel"], r)      # noqa: E731
        at, h = f(0.1, 2.2), 1e-5
        assert at["observed"]
        gx = (f(0.1 + h, 2.2)["f"] - f(0.1 - h, 2.2)["f"]) / (2 * h)
        gy = (f(0.1, 2.2 + h)["f"] - f(0.1, 2.2 - h)["f"]) / (2 * h)
        Hx = -(f(0.1 + h, 2.2)["G"] - f(0.1 - h, 2.2)["G"]) / (2 * h)
        Hy = -(f(0.1, 2.2 + h)["G"] - f(0.1, 2.2 - h)["G"]) / (2 * h)
        print(f"gene {g}: gradient {at['G']} against ({gx:.8g}, {gy:.8g}); observed matrix row x {at['M'][0]} against {Hx}")
        assert np.abs(np.array([gx, gy]) - at["G"]).max() <= 1e-6 * np.abs(at["G"]).max()
        assert np.abs(np.stack([Hx, Hy]) - at["M"]).max() <= 1e-6 * np.abs(at["M"]).max()


def _differences(p, v, h=1e-4):
    at = Q.profile64(p, v)
    for i in range(len(v)):
        e = np.zeros(len(v))
        e[i] = h
        up, dn = Q.profile64(p, v + e), Q.profile64(p, v - e)
        assert min(at["minz"], up["minz"], dn["minz"]) >= Q.MIN_Z                 # kink-free at every point visited
        yield i, at, (up["F"] - dn["F"]) / (2 * h), -(up["G"] - dn["G"]) / (2 * h)


@pytest.mark.parametrize("name", Q.OUTER_CASES + ["score_257_5_1", "score_257_5_3"])
def test_envelope_score_is_the_derivative_of_the_profiled_objective(name):
    """Central difference of F against the summed score, bar 1e-5 relative (a score is measured against the larger of itself and its
    own standard deviation sqrt(J_ii)); away from the optimum, where the score is not small."""
    p = Q.cases()[name]
    v = Q.outer_solved(name)[0]["nuw"] * 0.9 if name in Q.OUTER_CASES else p["nuw"]
    for i, at, fd, _ in _differences(p, v):
        scale = max(abs(at["G"][i]), np.sqrt(at["J"][i, i]))
        print(f"{name} coefficient {i}: score {at['G'][i]:.8g}, central difference {fd:.8g} (relative {abs(fd - at['G'][i]) / scale:.3g})")
        assert abs(fd - at["G"][i]) <= 1e-5 * scale


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_profile_information_is_minus_the_derivative_of_the_score(name):
    """At the reference's optimum (where the residuals have mean zero and the Fisher information stands for the observed), bar 1 %."""
    p = Q.cases()[name]
    for i, at, _, dG in _differences(p, Q.outer_solved(name)[0]["nuw"]):
        rel = np.abs(dG - at["J"][i]).max() / at["J"][i, i]
        print(f"{name} coefficient {i}: information {at['J'][i]}, -d score {dG} (relative {rel:.3g})")
        assert rel <= 0.01


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_reference_recovers_the_simulated_speed(name):
    p = Q.cases()[name]
    m64, m32, trace = Q.outer_solved(name)
    z = (m64["nuw"] - p["nuw"]) / m64["std"]
    print(f"{name}: nuw {m64['nuw']} +- {m64['std']} ({z} se from {p['nuw']}), {m64['rounds']} rounds; restatement {m32['nuw']}, "
          f"{m32['rounds']} rounds; min z over the trace {min(t[1] for t in trace):.3g}")
    assert m64["status"] == "CONVERGED" and m32["status"] == "CONVERGED" and m64["n_excluded"] == m32["n_excluded"] == 0
    assert np.abs(z).max() <= 4.0
    assert min(t[1] for t in trace) >= Q.MIN_Z
    for f, x, y in zip(m64["fits"], p["x"], p["y"]):
        s = np.sqrt(np.diag(f["inv"]))
        assert abs(f["x"] - x) <= 5 * s[0] and abs(f["y"] - y) <= 5 * s[1]


def test_fixtures_are_kink_free_or_kinked_as_declared():
    for name in Q.FIT_CASES + Q.SCORE_CASES:
        assert min(f64["minz"] for f64, _ in Q.solved(name)) >= Q.MIN_Z, name
    for name in Q.KINK_CASES:
        p = Q.cases()[name]
        Nc = p["U"].shape[0]
        frac = np.mean([f32["n_clamped"] / Nc for _, f32 in Q.solved(name)])
        print(f"{name}: {100 * frac:.1f} % of the cells clamped at the restatement's points")
        assert 0.10 <= frac <= 0.20
    retries = [(f64["fisher_retries"], f32["fisher_retries"]) for f64, f32 in Q.solved("confounded")]
    print("confounded: observed steps out of the box replaced by Fisher steps (reference, restatement):", retries)
    assert sum(a for a, _ in retries) >= 2 and sum(b for _, b in retries) >= 2
    assert Q.cases()["large_u16"]["U"].max() >= 2e4 and Q.cases()["large_u16"]["U"].max() <= 65535
    assert Q.cases()["large_f32"]["U"].max() > 65535
    print("bars:", {k: f"{v:.3g}" for k, v in Q.bars().items()})


def small():
    p = Q.cases()["shape_65_4_2_Poisson"]
    return p["U"].astype(np.float32), Q.directions(p["phis"]), p["n"], p["nu"].T


def test_check_arguments_refuses_by_name():
    from velocycle_amd.gene_kinetics import _check_omega, check_arguments, omega_design
    U, xy, n, means = small()
    ok = check_arguments(U, xy, n, means, 1, "NegativeBinomial", 0.3)
    assert ok[0].shape == (5, 65) and ok[2].shape == (4, 5) and ok[3].shape == (4,) and ok[4].shape == (4, 4) and ok[5] is None
    with pytest.raises(NotImplementedError):
        check_arguments(U, xy, n, means, noisemodel="Lognormal")
    seven = np.zeros((7, 4))
    for bad, msg in ((dict(means=seven), "3 are not instantiated"), (dict(means=means[:1]), "0 have no velocity"),
                     (dict(means=means[:, :3]), "means has 3 genes"), (dict(directions=xy[:, :-1]), "directions must be"),
                     (dict(directions=xy * 0), "non-zero length"), (dict(n_scounts=n[:-1]), "n_scounts has"),
                     (dict(n_scounts=-n), "n_scounts > 0"), (dict(tol=-1.0), "tol must be"), (dict(max_iter=0), "max_iter must be"),
                     (dict(noisemodel="NegativeBinomial", dispersion=-1.0), "dispersion must be > 0"),
                     (dict(noisemodel="NegativeBinomial", dispersion=np.ones(3)), "dispersion must be a scalar"),
                     (dict(prior=(0, 1, 2)), "the prior is"), (dict(prior=(0, -1, 2, 3)), "standard deviations"),
                     (dict(prior=(0, np.ones(3), 2, 3)), "the prior's entries"), (dict(evaluate_only=True), "evaluate_only needs start"),
                     (dict(start=np.zeros((3, 4))), "start must be"),
                     (dict(counts=U[0]), "counts must be")):
        kw = dict(counts=U, directions=xy, n_scounts=n, means=means)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            check_arguments(**kw)
    with pytest.raises(ValueError, match="omega must be a scalar"):
        _check_omega(np.ones(3), 65)
    with pytest.raises(ValueError, match="omega must be finite"):
        _check_omega(np.inf, 65)
    with pytest.raises(ValueError, match="at most 3"):
        omega_design(xy, 1, np.ones((2, 65)))
    with pytest.raises(ValueError, match="condition_design must be"):
        omega_design(xy, 0, np.ones((2, 64)))
    W = omega_design(xy, 1, None)
    assert np.allclose(W, Q.design64(Q.cases()["shape_65_4_2_Poisson"]["phis"], 1), atol=1e-14)


def test_container_signature_and_round_trip(monkeypatch):
    from velocycle_amd import gene_kinetics as GK
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import AngularSpeed, Cycle, Phases
    sig = inspect.signature(AngularSpeed.from_kinetics_mle)
    names = list(sig.parameters)
    assert names == ["cycle", "phases", "data", "harmonics", "condition_design", "noisemodel", "dispersion", "layer", "prior", "return_fit",
                     "worker_kw"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("layer", "prior", "return_fit"))
    assert sig.parameters["layer"].default == "unspliced" and sig.parameters["harmonics"].default == 0
    U, xy, n, means = small()
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(65)])
    ad = AnnDataLite(U * 2, U, gene_names=[f"g{i}" for i in range(4)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    cyc = Cycle.from_array(means, np.ones_like(means), gene_names=list(ad.var.index))
    seen = {}

    def fake(counts, directions, n_scounts, means_, **kw):
        seen.update(kw, counts=counts, means=means_)
        kin = GK.GeneKineticsFit(*[np.arange(4.0)] * 2, *[None] * 9)
        return GK.VelocityMapFit(nu_omega=np.array([[0.4, 0.3]]), stds=np.array([[0.04, 0.03]]), cov=np.eye(2), F=0.0, dec=0.0, rounds=1,
                                 status="CONVERGED", n_excluded=0, included=np.ones(4, bool), kinetics=kin)
    monkeypatch.setattr(GK, "velocity_map", fake)
    D = np.zeros((2, 65))
    D[0, :30], D[1, 30:] = 1, 1
    prior = AngularSpeed.trivial_prior(["a", "b"], harmonics=0)
    out, fit = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, D, "NegativeBinomial", 0.2, prior=prior, return_fit=True, max_rounds=7)
    assert seen["counts"] is not None and np.array_equal(seen["counts"], U) and seen["max_rounds"] == 7 and seen["nuw_prior"] is prior
    assert seen["noisemodel"] == "NegativeBinomial" and seen["dispersion"] == 0.2 and seen["harmonics_w"] == 0
    assert out.conditions == ["a", "b"] and out.means.shape == (1, 2) and list(out.means.index) == ["nu0"]
    assert np.array_equal(out.means.values, fit.nu_omega) and np.array_equal(out.stds.values, fit.stds)
    new = fit.to_cycle(cyc)
    assert new is not cyc and cyc.log_gammas is None and np.array_equal(new.log_gammas, np.arange(4.0))
    assert np.array_equal(new.log_betas, np.arange(4.0)) and new.means.equals(cyc.means)
    with pytest.raises(ValueError, match="cells of the phases"):
        AngularSpeed.from_kinetics_mle(cyc, Phases.from_array(xy[:, :-1]), ad)
    with pytest.raises(ValueError, match="genes of the cycle"):
        AngularSpeed.from_kinetics_mle(Cycle.from_array(means[:, :3], means[:, :3]), ph, ad)
    with pytest.raises(ValueError, match="is not a layer"):
        AngularSpeed.from_kinetics_mle(cyc, ph, ad, layer="nope")
    with pytest.raises(NotImplementedError):
        AngularSpeed.from_kinetics_mle(cyc, ph, ad, noisemodel="Lognormal")


def test_header_declares_and_lib_binds_vc_gene_kinetics():
    from velocycle_amd import _lib
    from velocycle_amd.gene_kinetics import STATUS
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert " *   vc_gene_kinetics " in hdr and "#define VC_ABI_VERSION 2" in hdr
    for i, name in enumerate(["CONVERGED", "ROUNDING", "MAX_ITER", "UNBOUNDED", "NO_DATA", "EVALUATED"]):
        assert f"#define VC_KIN_{name} {i}" in hdr and getattr(_lib, f"VC_KIN_{name}") == i == getattr(Q, name) and STATUS[i] == name
    decl = re.search(r"\bint vc_gene_kinetics\(([^;]*)\);", hdr).group(1)
    assert len(_lib.EXPORTS["vc_gene_kinetics"][1]) == len(decl.split(",")) == 28 and decl.rstrip().endswith("void* hip_stream")
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_kinetics.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace {")[1]
    assert f"KIN_BOUND = {Q.BOUND};" in src and f"KIN_MAX_HALVINGS = {Q.HALVINGS};" in src and "KIN_FLOOR = 1.0e-5;" in src


def kin_args(**k):
    """Arguments of vc_gene_kinetics with pointers that are never dereferenced: every call made with them is refused before the launch."""
    one = C.c_void_p(64)
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("nu", one), k.get("w", one), k.get("NW", 1), k.get("nuw", one), k.get("noise", 1), k.get("r", None),
            k.get("prior", one), k.get("start", None), k.get("tol", 1e-10), k.get("max_iter", 25), k.get("xy", one), k.get("cov", one),
            k.get("ll", one), k.get("dec", one), k.get("it", one), k.get("st", one), k.get("nc", one), k.get("score", one),
            k.get("info", one), None]


REFUSALS = [(dict(K=K), b"K must be 3 or 5") for K in (0, 1, 2, 4, 9)] + [(dict(K=7), b"H = 3")] + \
    [({name: None}, b"null") for name in ("counts", "basis", "logm", "nu", "prior", "xy", "cov", "ll", "dec", "it", "st", "nc")] + \
    [(dict(NW=-1), b"NW must be"), (dict(NW=4), b"NW must be"), (dict(w=None), b"w_dev and nuw_dev"), (dict(nuw=None), b"w_dev and nuw_dev"),
     (dict(score=None), b"NW outputs"), (dict(info=None), b"NW outputs"), (dict(noise=0), b"r_dev"), (dict(noise=5), b"noise must be"),
     (dict(Nc=0), b"Nc"), (dict(Ng=0), b"Ng"), (dict(Nc=1 << 31, stride=1 << 31), b"2^31"), (dict(stride=3), b"gene_stride"),
     (dict(max_iter=-1), b"max_iter"), (dict(max_iter=0), b"start_dev"), (dict(tol=-1e-3), b"tol"), (dict(tol=float("nan")), b"tol"),
     (dict(kind=7), b"count_kind")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for kw, msg in REFUSALS:
        assert lib.vc_gene_kinetics(*kin_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_kinetics(*kin_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    # in each of the four per-gene entry points the shared refusals and every refusal of its own come before the launch
    for name in ("vc_gene_glm", "vc_gene_glm_batch", "vc_gene_dispersion", "vc_gene_kinetics"):
        src = open(os.path.join(ROOT, "velocycle_amd", "csrc", name + ".hip")).read()
        body = src[src.index(f'extern "C" int {name}('):]
        launch = body.index("hipLaunchKernelGGL")
        assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < launch, name
        assert body.rindex("gene_fail(") < launch < body.index("gene_launched("), name


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_gene_kinetics_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly emitted for
    gfx950 (hipcc -S --cuda-device-only), fits two workgroups of 256 lanes to a SIMD's registers, and uses under 1 KiB of LDS."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_kinetics.hip")
    out = str(tmp_path / "kin.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*vc_gene_kinetics_kernel\S*)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(found) == 32, len(found)                    # H {1, 2} x NW 0..3 x {NB, Poisson} x {u16, f32}
    print("VGPRs:", sorted({int(v) for _, _, _, v in found}))
    assert all(int(p) == 0 for _, _, p, _ in found), found
    assert all(int(lds) <= 1024 and int(v) <= 256 for lds, _, _, v in found), found
