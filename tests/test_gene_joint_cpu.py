"""CPU: the joint fit's float64 reference against finite differences and the simulated truth, the float32 restatement against the
reference, every refusal that needs no device, and what the header, the binding, the kernel source and the code object say.  Measured
values are printed by every test and written into its docstring."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import gene_joint_checker as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _at(p, g):
    kS, kU, B, logm, r = Q.gene_inputs(p, g)
    return lambda th: Q.point64(th, kS, kU, B, logm, p["W"], p["nuw"], p["noisemodel"], r)      # noqa: E731


def test_db_is_the_derivative_basis():
    phis = np.linspace(0.1, 6.0, 17)
    for H in (1, 2):
        assert np.abs(Q.db_from_basis(Q.basis64(phis, H)) - Q.dbasis64(phis, H)).max() <= 1e-15


@pytest.mark.parametrize("name,g", [("shape_257_5_1_NegativeBinomial", 0), ("shape_257_5_2_Poisson", 3), ("score_1025_3_3", 1)])
def test_gradient_and_observed_matrix_are_the_derivatives_of_f(name, g):
    """Central differences (h = 1e-5) at a point 0.05 off the truth in every parameter, bar 1e-6 relative to the largest entry (the
    ceiling of the kinetics tests).  Measured: gradient 1e-10 .. 6e-10, observed matrix 2e-11 .. 4e-11."""
    p = Q.cases()[name]
    f = _at(p, g)
    th = Q.truth(p, g) + 0.05
    at, h = f(th), 1e-5
    assert at["minz"] >= Q.MIN_Z
    fd_g, fd_O = np.zeros_like(th), np.zeros((len(th), len(th)))
    for i in range(len(th)):
        e = np.zeros(len(th))
        e[i] = h
        up, dn = f(th + e), f(th - e)
        fd_g[i] = (up["f"] - dn["f"]) / (2 * h)
        fd_O[i] = -(up["G"] - dn["G"]) / (2 * h)
    rel_g, rel_O = np.abs(fd_g - at["G"]).max() / np.abs(at["G"]).max(), np.abs(fd_O - at["O"]).max() / np.abs(at["O"]).max()
    print(f"{name} gene {g}: gradient off by {rel_g:.3g}, observed matrix by {rel_O:.3g} (relative to the largest entry)")
    assert rel_g <= 1e-6 and rel_O <= 1e-6
    assert np.abs(at["O"] - at["O"].T).max() <= 1e-13 * np.abs(at["O"]).max() and np.linalg.eigvalsh(at["F"]).min() > 0


def _differences(p, v, genes, h=1e-4, starts=None):
    """starts: None (every gene from the default start), or a start per gene (an outer case's genes start at its optimum's theta: a
    first full step from the flat start crosses the kink in some of 30-40 genes, and F does not depend on the start)."""
    at = Q.profile64(p, v, genes, starts)
    for i in range(len(v)):
        e = np.zeros(len(v))
        e[i] = h
        up, dn = Q.profile64(p, v + e, genes, starts), Q.profile64(p, v - e, genes, starts)
        assert min(at["minz"], up["minz"], dn["minz"]) >= Q.MIN_Z                 # kink-free at every point visited
        yield i, at, (up["F"] - dn["F"]) / (2 * h), -(up["G"] - dn["G"]) / (2 * h)


@pytest.mark.parametrize("name", Q.OUTER_CASES + ["score_257_5_1", "score_257_5_3"])
def test_envelope_score_is_the_derivative_of_the_profiled_objective(name):
    """Central difference of F against the summed score, bar 1e-5 relative (a score is measured against the larger of itself and its
    own standard deviation sqrt(J_ii)); away from the optimum, where the score is not small.  Measured: at most 1e-6."""
    p = Q.cases()[name]
    outer = name in Q.OUTER_CASES
    v = Q.outer_solved(name)[0]["nuw"] * 0.9 if outer else p["nuw"]
    starts = [f["th"] for f in Q.outer_solved(name)[0]["fits"]] if outer else None
    for i, at, fd, _ in _differences(p, v, range(min(p["U"].shape[1], 10)), starts=starts):
        scale = max(abs(at["G"][i]), np.sqrt(at["J"][i, i]))
        print(f"{name} coefficient {i}: score {at['G'][i]:.8g}, central difference {fd:.8g} (relative {abs(fd - at['G'][i]) / scale:.3g})")
        assert abs(fd - at["G"][i]) <= 1e-5 * scale


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_profile_information_is_minus_the_derivative_of_the_score(name):
    """At the reference's optimum (where the residuals have mean zero and the Fisher information stands for the observed), bar 1 %
    over all genes of the case (the bar of the kinetics tests).  Measured: 0.02 .. 0.22 %."""
    p = Q.cases()[name]
    m64 = Q.outer_solved(name)[0]
    for i, at, _, dG in _differences(p, m64["nuw"], None, starts=[f["th"] for f in m64["fits"]]):
        rel = np.abs(dG - at["J"][i]).max() / at["J"][i, i]
        print(f"{name} coefficient {i}: information {at['J'][i]}, -d score {dG} (relative {rel:.3g})")
        assert rel <= 0.01


def test_every_simulated_parameter_is_within_four_standard_errors():
    """The five shapes of the prototype; 4 is the bar the kinetics tests use.  Measured worst: 2.75 (the prototype's own: 2.7)."""
    worst = 0.0
    for name, p in Q.recovery_cases().items():
        fits = Q._solved(p)
        Q.assert_kink_free(name, fits)
        for g, (f64, f32) in enumerate(fits):
            assert f64["status"] == Q.CONVERGED and f32["status"] in Q.INTERIOR and 4 <= f64["iterations"] <= 12
            z = (f64["th"] - Q.truth(p, g)) / np.sqrt(np.diag(f64["inv"]))
            worst = max(worst, np.abs(z).max())
        print(f"{name}: steps {[f64['iterations'] for f64, _ in fits]}, worst so far {worst:.3g} se")
    assert worst <= 4.0


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


def test_restatement_takes_the_reference_s_steps():
    """The restatement stops (dec <= tol, or the rounding rule) within one step of the reference's first dec <= tol."""
    for name in Q.FIT_CASES + Q.SCORE_CASES:
        for g, (f64, f32) in enumerate(Q.solved(name)):
            assert f64["first_tol"] is not None and abs(f32["iterations"] - f64["first_tol"]) <= 1, (name, g, f32["iterations"], f64["first_tol"])


def test_fixtures_are_kink_free_or_kinked_as_declared():
    for name in Q.FIT_CASES + Q.SCORE_CASES:
        Q.assert_kink_free(name, Q.solved(name))
    Nc = Q.cases()["kink_a"]["U"].shape[0]
    frac = np.mean([f32["n_clamped"] / Nc for _, f32 in Q.solved("kink_a")])
    print(f"kink_a: {100 * frac:.1f} % of the cells clamped at the restatement's points")
    assert frac >= 0.05
    assert 2e4 <= Q.cases()["large_u16"]["U"].max() <= 65535 and Q.cases()["large_f32"]["U"].max() > 65535
    assert sum(Q.evaluated()[(4, g)][1]["n_clamped"] for g in range(5)) > 0
    print("bars:", {k: f"{v:.3g}" for k, v in Q.bars().items()})


def small():
    p = Q.cases()["shape_65_4_2_Poisson"]
    return p["S"].astype(np.float32), p["U"].astype(np.float32), Q.directions(p["phis"]), p["n"]


def test_check_arguments_refuses_by_name():
    from velocycle_amd.gene_joint import _design, check_arguments
    from velocycle_amd.gene_kinetics import GeneKineticsFit
    S, U, xy, n = small()
    ok = check_arguments(S, U, xy, n, 2, 1, "NegativeBinomial", 0.3)
    assert ok[0].shape == (5, 65) and ok[2].shape == (4,) and ok[3].shape == ok[4].shape == (4, 5) and ok[5].shape == (4, 4) and ok[6] is None
    assert (ok[3] == 0).all() and np.allclose(ok[4], 1 / 9)
    with pytest.raises(NotImplementedError):
        check_arguments(S, U, xy, n, noisemodel="Lognormal")
    with pytest.raises(NotImplementedError, match="Δν"):
        check_arguments(S, U, xy, n, batch_design=np.ones((65, 2)))
    with pytest.raises(NotImplementedError, match="case weights"):
        check_arguments(S, U, xy, n, cell_weights=np.ones(65))
    with pytest.raises(TypeError):
        check_arguments(S, U, xy, n, nonsense=1)
    means = np.zeros((5, 4))
    for bad, msg in ((dict(harmonics=3), "3 are not instantiated"), (dict(harmonics=0), "0 have no velocity"),
                     (dict(counts_U=U[:, :3]), "counts_U must be"), (dict(directions=xy[:, :-1]), "directions must be"),
                     (dict(directions=xy * 0), "non-zero length"), (dict(n_scounts=n[:-1]), "n_scounts has"),
                     (dict(n_scounts=-n), "n_scounts > 0"), (dict(tol=-1.0), "tol must be"), (dict(max_iter=0), "max_iter must be"),
                     (dict(noisemodel="NegativeBinomial", dispersion=-1.0), "dispersion must be > 0"),
                     (dict(prior_means=means), "both prior_means and prior_stds"), (dict(prior_means=means[:3], prior_stds=means[:3] + 1), "must be"),
                     (dict(prior_means=means, prior_stds=means), "finite and > 0"),
                     (dict(prior_means=means + np.nan, prior_stds=means + 1), "finite and > 0"),
                     (dict(kinetics_prior=(0, 1, 2)), "kinetics_prior is"), (dict(kinetics_prior=(0, -1, 2, 3)), "standard deviations"),
                     (dict(kinetics_prior=(0, np.ones(3), 2, 3)), "kinetics_prior's entries"),
                     (dict(evaluate_only=True), "evaluate_only needs start"), (dict(start=np.zeros((7, 4))), "start must be"),
                     (dict(start=(means, np.zeros(3), np.zeros(4))), "start must be"), (dict(counts_S=S[0]), "counts must be")):
        kw = dict(counts_S=S, counts_U=U, directions=xy, n_scounts=n, harmonics=2)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            check_arguments(**kw)
    kin = GeneKineticsFit(np.arange(4.0), np.arange(4.0) + 1, *[None] * 9)
    for start in ((means + 1, kin), (kin, means + 1), (means + 1, np.arange(4.0), np.arange(4.0) + 1)):
        st = check_arguments(S, U, xy, n, 2, start=start)[6]
        assert st.shape == (4, 7) and (st[:, :5] == 1).all() and np.array_equal(st[:, 5], np.arange(4.0)) and np.array_equal(st[:, 6], np.arange(4.0) + 1)
    with pytest.raises(ValueError, match="either omega"):
        _design(xy, 65, None, None, 0, None)
    with pytest.raises(ValueError, match="either omega"):
        _design(xy, 65, 0.4, [0.4], 0, None)
    with pytest.raises(ValueError, match="at most 3"):
        _design(xy, 65, None, np.ones(6), 1, np.ones((2, 65)))
    with pytest.raises(ValueError, match="nu_omega must be"):
        _design(xy, 65, None, np.ones(2), 1, None)
    W, nuw = _design(xy, 65, 0.4, None, 0, None)
    assert W.shape == (1, 65) and (W == 0.4).all() and nuw.tolist() == [1.0]


def test_container_signatures_and_round_trip(monkeypatch):
    import pandas as pd

    import velocycle_amd
    from velocycle_amd import gene_joint as GJ
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import AngularSpeed, Cycle, Phases
    assert {"velocity_map_joint", "GeneJointFit", "JointVelocityMapFit"} <= set(velocycle_amd.__all__)
    assert velocycle_amd.velocity_map_joint is GJ.velocity_map_joint and velocycle_amd.JointVelocityMapFit is GJ.JointVelocityMapFit
    assert velocycle_amd.gene_joint is GJ and velocycle_amd.GeneJointFit is GJ.GeneJointFit      # gene_joint is its module's name
    names = list(inspect.signature(GJ.gene_joint).parameters)
    assert names[:9] == ["counts_S", "counts_U", "directions", "n_scounts", "omega", "harmonics", "a", "noisemodel", "dispersion"]
    assert names[9:21] == ["prior_means", "prior_stds", "kinetics_prior", "start", "evaluate_only", "tol", "max_iter", "device", "chunk_genes",
                           "storage", "nu_omega", "harmonics_w"] and names[21] == "condition_design"
    assert inspect.signature(GJ.gene_joint).parameters["max_iter"].default == 40
    assert list(inspect.signature(Cycle.from_joint_mle).parameters)[:3] == ["phases", "data", "angular_speed"]
    assert list(inspect.signature(AngularSpeed.from_joint_mle).parameters)[:3] == ["cycle_prior", "phases", "data"]
    S, U, xy, n = small()
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(65)])
    ad = AnnDataLite(S, U, gene_names=[f"g{i}" for i in range(4)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    seen = {}
    fit = GJ.GeneJointFit(means=np.ones((5, 4)), log_gamma=np.arange(4.0), log_beta=np.arange(4.0) + 1, cov=None, stds=np.full((7, 4), 0.5),
                          **{k: None for k in ("loglik_S", "loglik_U", "decrement", "iterations", "status", "n_clamped", "score_w", "info_w")})

    def fake_map(cS, cU, directions, n_scounts, **kw):
        seen.update(kw, S=cS, U=cU)
        return GJ.JointVelocityMapFit(nu_omega=np.array([[0.4, 0.3]]), stds=np.array([[0.04, 0.03]]), cov=np.eye(2), F=0.0, dec=0.0, rounds=1,
                                      status="CONVERGED", n_excluded=0, included=np.ones(4, bool), genes=fit)

    def fake_fit(cS, cU, directions, n_scounts, **kw):
        seen.clear()
        seen.update(kw, S=cS, U=cU)
        return fit
    monkeypatch.setattr(GJ, "velocity_map_joint", fake_map)
    monkeypatch.setattr(GJ, "gene_joint", fake_fit)
    D = np.zeros((2, 65))
    D[0, :30], D[1, 30:] = 1, 1
    prior = AngularSpeed.trivial_prior(["a", "b"], harmonics=0)
    cyc_prior = Cycle.trivial_prior(list(ad.var.index), harmonics=2)
    out, mfit = AngularSpeed.from_joint_mle(cyc_prior, ph, ad, 0, D, "NegativeBinomial", 0.2, prior=prior, return_fit=True, max_rounds=7)
    assert np.array_equal(seen["S"], S) and np.array_equal(seen["U"], U) and seen["max_rounds"] == 7 and seen["nuw_prior"] is prior
    assert seen["harmonics"] == 2 and seen["harmonics_w"] == 0 and np.array_equal(seen["prior_stds"], cyc_prior.stds.values)
    assert out.conditions == ["a", "b"] and np.array_equal(out.means.values, mfit.nu_omega)
    new = mfit.to_cycle(cyc_prior)
    assert new is not cyc_prior and cyc_prior.log_gammas is None and np.array_equal(new.log_gammas, np.arange(4.0))
    assert (new.means.values == 1).all() and (new.stds.values == 0.5).all() and (cyc_prior.means.values == 0).all()
    cyc = Cycle.from_joint_mle(ph, ad, out, 2, D, tol=1e-9)
    assert seen["tol"] == 1e-9 and seen["nu_omega"].tolist() == [0.4, 0.3] and seen["harmonics_w"] == 0 and seen["condition_design"] is D
    assert seen["prior_means"] is None and list(cyc.means.columns) == list(ad.var.index) and np.array_equal(cyc.log_betas, np.arange(4.0) + 1)
    Cycle.from_joint_mle(ph, ad, 0.4, 2)
    assert seen["omega"] == 0.4 and "nu_omega" not in seen
    with pytest.raises(ValueError, match="cells of the phases"):
        Cycle.from_joint_mle(Phases.from_array(xy[:, :-1]), ad, 0.4)
    with pytest.raises(ValueError, match="the prior has 2 harmonics"):
        Cycle.from_joint_mle(ph, ad, 0.4, 1, prior=cyc_prior)
    with pytest.raises(NotImplementedError):
        AngularSpeed.from_joint_mle(None, ph, ad, noisemodel="Lognormal")


def test_header_declares_and_lib_binds_vc_gene_joint():
    from velocycle_amd import _lib
    from velocycle_amd.gene_joint import STATUS
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert " *   vc_gene_joint " in hdr and "#define VC_ABI_VERSION 2" in hdr
    for i, name in enumerate(["CONVERGED", "ROUNDING", "MAX_ITER", "UNBOUNDED", "NO_DATA", "EVALUATED"]):
        assert f"#define VC_JNT_{name} {i}" in hdr and getattr(_lib, f"VC_JNT_{name}") == i == getattr(Q, name) and STATUS[i] == name
        assert getattr(_lib, f"VC_KIN_{name}") == i                # numbered like VC_KIN_*
    decl = re.search(r"\bint vc_gene_joint\(([^;]*)\);", hdr).group(1)
    assert len(_lib.EXPORTS["vc_gene_joint"][1]) == len(decl.split(",")) == 31 and decl.rstrip().endswith("void* hip_stream")
    assert decl.split(",")[0].strip() == "const void* counts_s_dev" and decl.split(",")[1].strip() == "const void* counts_u_dev"
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace {")[1]
    assert f"JNT_BOUND = {Q.XY_BOUND};" in src and f"JNT_MAX_HALVINGS = {Q.HALVINGS};" in src and "JNT_FLOOR = 1.0e-5;" in src
    glm = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_glm_math.h")).read()
    assert f"GLM_BOUND = {Q.NU_BOUND};" in glm


def jnt_args(**k):
    """Arguments of vc_gene_joint with pointers that are never dereferenced: every call made with them is refused before the launch."""
    one = C.c_void_p(64)
    return [k.get("counts_s", one), k.get("counts_u", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4),
            k.get("basis", one), k.get("K", 3), k.get("logm", one), k.get("w", one), k.get("NW", 1), k.get("nuw", one), k.get("noise", 1),
            k.get("r", None), k.get("pm", one), k.get("pp", one), k.get("prior", one), k.get("start", None), k.get("tol", 1e-10),
            k.get("max_iter", 25), k.get("theta", one), k.get("cov", one), k.get("lls", one), k.get("llu", one), k.get("dec", one),
            k.get("it", one), k.get("st", one), k.get("nc", one), k.get("score", one), k.get("info", one), None]


REFUSALS = [(dict(K=K), b"K must be 3 or 5") for K in (0, 1, 2, 4, 9)] + [(dict(K=7), b"H = 3")] + \
    [({name: None}, b"null") for name in ("counts_s", "counts_u", "basis", "logm", "prior", "pm", "pp", "theta", "cov", "lls", "llu", "dec", "it",
                                          "st", "nc")] + \
    [(dict(NW=-1), b"NW must be"), (dict(NW=4), b"NW must be"), (dict(w=None), b"w_dev and nuw_dev"), (dict(nuw=None), b"w_dev and nuw_dev"),
     (dict(score=None), b"NW outputs"), (dict(info=None), b"NW outputs"), (dict(NW=0, w=None, nuw=None), b"need NW > 0"),
     (dict(NW=0, w=None, nuw=None, score=None), b"need NW > 0"), (dict(noise=0), b"r_dev"), (dict(noise=5), b"noise must be"),
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
        assert lib.vc_gene_joint(*jnt_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_joint(*jnt_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint.hip")).read()
    body = src[src.index('extern "C" int vc_gene_joint('):]
    launch = body.index("hipLaunchKernelGGL")
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < launch
    assert body.rindex("gene_fail(") < launch < body.index("gene_launched(")


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_gene_joint_kernel (H {1, 2} x NW 0..3 x NB / Poisson x uint16 / float32 = 32) reports
    .private_segment_fixed_size 0 in the metadata of the assembly emitted for gfx950 (hipcc -S --cuda-device-only).  Measured: LDS
    1160 .. 2320 bytes (five rows of the longest fold: 29 sums at H = 1 without the profile pass, 58 at H = 2 with NW = 3), 200 .. 300
    VGPRs (accumulation registers included: one workgroup of 256 lanes per SIMD set fits; 512 are there)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_gene_joint.hip")
    out = str(tmp_path / "jnt.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*vc_gene_joint_kernel\S*)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(found) == 32, len(found)
    print("VGPRs:", sorted({int(v) for _, _, _, v in found}), "LDS bytes:", sorted({int(lds) for lds, _, _, _ in found}))
    assert all(int(p) == 0 for _, _, p, _ in found), found
    assert all(int(lds) <= 2320 and int(v) <= 512 for lds, _, _, v in found), found
    assert {int(lds) for lds, _, _, _ in found} == {5 * 8 * n for n in (29, 30, 39, 46, 47, 58)}
