"""CPU: the checker of the per-cell and per-group angular speed (tests/cell_speed_checker.py) against finite differences, the
simulation's truth and its own restatement; the host side of `velocycle_amd.cell_speed` (refusals before any device work, the group
sums' order, the host iteration over groups, `phase_bin_groups`); the C ABI declaration, its binding and its refusals; the kernel's code
object.  Every test prints the figures it asserts on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cell_speed_checker as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_and_observed_information_are_the_derivatives_of_L():
    for name, c in (("shape_65_64_1_Poisson", 3), ("shape_64_65_2_NegativeBinomial", 10), ("shape_1_257_2_NegativeBinomial", 0)):
        for om in (0.4, 0.1):
            at, h = Q.at64(name, [c], om), 1e-5
            lo, hi = Q.at64(name, [c], om - h), Q.at64(name, [c], om + h)
            fd1, fd2 = (hi["L"] - lo["L"]) / (2 * h), (hi["score"] - lo["score"]) / (2 * h)
            print(f"{name} cell {c} at {om}: score {at['score']:.8g} (difference {fd1:.8g}), observed {at['observed']:.8g} ({-fd2:.8g}), "
                  f"fisher {at['fisher']:.8g}, min z {at['minz']:.3g}")
            assert at["minz"] > 0.05
            assert abs(fd1 - at["score"]) <= 1e-5 * max(1.0, abs(at["score"]), at["fisher"])
            assert abs(-fd2 - at["observed"]) <= 1e-6 * at["fisher"]
    # a prior adds its own terms to G and to the matrix, and nothing to the sums
    with_prior, without = Q.at64("shape_65_64_1_Poisson", [3], 0.4, (0.1, 2.0)), Q.at64("shape_65_64_1_Poisson", [3], 0.4)
    assert with_prior["score"] == without["score"] and with_prior["G"] == without["score"] - (0.4 - 0.1) / 4.0
    assert with_prior["M"] == without["observed"] + 0.25 and with_prior["f"] == without["L"] - 0.5 * 0.09 / 4.0


def test_cases_are_kink_free_and_converge():
    """What the tolerance-bearing cases promise of the float64 reference: min z >= 0.05 over every point visited, >= 90 % CONVERGED."""
    for name in Q.FIT_CASES:
        conv = Q.check_case(name)
        sol = Q.solved(name)
        minz = min(f64["minz_path"] for f64, _ in sol if f64["status"] != Q.NO_DATA)
        print(f"{name}: min z {minz:.3g}, {len(conv)} of {len(sol)} CONVERGED, at most {max(f64['iterations'] for f64, _ in sol)} steps "
              f"(restatement {max(f32['iterations'] for _, f32 in sol)})")
    kink = Q.solved(Q.KINK_CASE)
    minz = min(f64["minz_path"] for f64, _ in kink)
    print(f"{Q.KINK_CASE}: min z {minz:.3g}, omega {min(f['om'] for f, _ in kink):.3g} .. {max(f['om'] for f, _ in kink):.3g}")
    assert minz < 0                                                # the kink case kinks
    top = {name: Q.cases()[name]["U"].max() for name in Q.LARGE_CASES}
    assert 2e4 <= top["large_u16"] <= 65535 < top["large_f32"], top


def test_calibration_of_the_fisher_standard_error():
    """65 x 64, H = 1, Poisson, kinetics at the truth, start 0.4: (omega_c - 0.4) / se_c is standard normal if the standard error is right."""
    sol = Q.solved("shape_65_64_1_Poisson")
    z = np.array([(f64["om"] - 0.4) / f64["se"] for f64, _ in sol])
    rms = float(np.sqrt((z ** 2).mean()))
    print(f"rms {rms:.3f}, worst {np.abs(z).max():.2f}, steps <= {max(f64['iterations'] for f64, _ in sol)}")
    assert 0.8 <= rms <= 1.25


def test_bins_recover_the_mean_true_speed():
    """Eight phase bins of 1025 x 12 (NB, nuw = (0.4, 0.1, -0.1), Hw = 1) and two conditions x four bins: each within 4 se of the mean
    true speed of its cells."""
    for name in Q.GROUP_CASES:
        p = Q.cases()[name]
        worst = 0.0
        for g, (f64, _, rows) in enumerate(Q.group_solved(name)):
            truth = Q.true_speed(p)[rows].mean()
            z = (f64["om"] - truth) / f64["se"]
            print(f"{name} group {g}: {len(rows)} cells, omega {f64['om']:.4f} +- {f64['se']:.4f}, truth {truth:.4f} ({z:+.2f} se), "
                  f"{f64['iterations']} steps")
            assert f64["status"] == Q.CONVERGED and f64["iterations"] <= 6
            worst = max(worst, abs(z))
        assert worst <= 4.0


def test_restatement_against_the_reference():
    """The float32 restatement lands on the reference's optimum to a small fraction of a standard error, in no more steps + 2."""
    bars = Q.bars()
    print({k: float(f"{v:.3g}") for k, v in bars.items()})
    assert bars["omega"] <= 1e-2 and bars["group"] <= 1e-2 and bars["var"] <= 1e-3 and bars["fisher"] <= 1e-3 and bars["observed"] <= 1e-3
    for name in Q.FIT_CASES:
        for c, f64, f32 in Q.check_case(name):
            assert f32["iterations"] <= f64["iterations"] + 2 and f32["n_clamped"] == 0
    for i in range(len(Q.EVALUATE_AT)):
        assert all(Q.evaluated()[(i, c)][0]["n_clamped"] == Q.evaluated()[(i, c)][1]["n_clamped"] for c in range(65))
    assert sum(Q.evaluated()[(4, c)][1]["n_clamped"] for c in range(65)) > 0


# ------------------------------------------------------------------------------------------------------------------ the host side
def host_args(name="shape_65_64_1_Poisson"):
    from tests.gene_kinetics_checker import directions
    p = Q.cases()[name]
    return p, (p["U"].astype(np.float32), directions(p["phis"]), p["n"], p["nu"].T.copy(), p["x"].copy(), p["y"].copy())


def test_refusals_need_no_device():
    from velocycle_amd import cell_speed as cs
    p, (U, xy, n, means, lg, lb) = host_args()
    Nc, Ng = U.shape
    with pytest.raises(NotImplementedError):
        cs.check_arguments(U, xy, n, means, lg, lb, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="3 are not instantiated"):
        cs.check_arguments(U, xy, n, np.zeros((7, Ng)), lg, lb)
    with pytest.raises(ValueError, match="one value per gene"):
        cs.check_arguments(U, xy, n, means, lg[:-1], lb)
    bad = lg.copy()
    bad[[2, 5]] = np.nan
    keep = cs.check_arguments(U, xy, n, means, bad, lb)[0]                     # the default mask drops them
    assert keep.tolist() == [g for g in range(Ng) if g not in (2, 5)]
    assert cs.check_arguments(U, xy, n, means, lg, lb)[0] is None
    with pytest.raises(ValueError, match="2 of the 64 kept genes"):
        cs.check_arguments(U, xy, n, means, bad, lb, genes=np.ones(Ng, dtype=bool))
    mask = np.ones(Ng, dtype=bool)
    mask[[2, 5, 9]] = False
    keep, basis, logm, nu, xk, r = cs.check_arguments(U, xy, n, means, bad, lb, noisemodel="NegativeBinomial", dispersion=0.25, genes=mask)
    assert len(keep) == Ng - 3 and nu.shape == (Ng - 3, 3) and xk.shape == (Ng - 3, 2) and r.shape == (Ng - 3,) and basis.shape == (3, Nc)
    assert np.array_equal(xk[:, 0], lg[mask]) and np.array_equal(nu, means.T[mask])
    with pytest.raises(ValueError, match="boolean mask"):
        cs.check_arguments(U, xy, n, means, lg, lb, genes=np.arange(Ng))
    with pytest.raises(ValueError, match="no gene is kept"):
        cs.check_arguments(U, xy, n, means, lg, lb, genes=np.zeros(Ng, dtype=bool))
    # everything below is refused before a device is asked for
    with pytest.raises(ValueError, match="start must be a scalar or one value per cell"):
        cs.cell_angular_speed(U, xy, n, means, lg, lb, np.zeros(3))
    with pytest.raises(ValueError, match="prior"):
        cs.cell_angular_speed(U, xy, n, means, lg, lb, 0.4, prior=(0.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="storage"):
        cs.cell_angular_speed(U, xy, n, means, lg, lb, 0.4, storage="u8")
    with pytest.raises(ValueError, match="chunk_cells"):
        cs.cell_angular_speed(U, xy, n, means, lg, lb, 0.4, chunk_cells=0)
    with pytest.raises(ValueError, match="one integer per cell"):
        cs.grouped_angular_speed(U, xy, n, means, lg, lb, np.zeros(Nc), 0.4)
    with pytest.raises(ValueError, match="n_groups"):
        cs.grouped_angular_speed(U, xy, n, means, lg, lb, np.arange(Nc), 0.4, n_groups=3)
    with pytest.raises(ValueError, match="sds > 0"):
        cs.grouped_angular_speed(U, xy, n, means, lg, lb, np.zeros(Nc, dtype=int), 0.4, prior=(0.0, 0.0))
    with pytest.raises(ValueError, match="max_rounds"):
        cs.grouped_angular_speed(U, xy, n, means, lg, lb, np.zeros(Nc, dtype=int), 0.4, max_rounds=-1)
    import velocycle_amd
    assert {"cell_angular_speed", "grouped_angular_speed", "CellSpeedFit", "GroupSpeedFit"} <= set(velocycle_amd.__all__)
    assert velocycle_amd.cell_angular_speed is cs.cell_angular_speed and velocycle_amd.GroupSpeedFit is cs.GroupSpeedFit
    for text in (cs.__doc__, cs.grouped_angular_speed.__doc__ + cs.CellSpeedFit.__doc__):
        assert "conditional" in text or "order of the cells' positions" in text
    assert "no p-value" in cs.__doc__ and "relu kink" in cs.__doc__ and "Δν" in cs.__doc__


def test_group_sums_add_in_the_order_of_the_cells():
    from velocycle_amd.cell_speed import group_sums
    rng = np.random.default_rng(3)
    Nc, G = 500, 7
    sums = rng.normal(size=(Nc, 6)) * 10.0 ** rng.integers(-8, 8, size=(Nc, 6))   # sums whose order of addition shows in the bits
    ncl = rng.integers(0, 5, Nc).astype(np.int32)
    ok = rng.uniform(size=Nc) > 0.1
    groups = rng.integers(0, G - 1, Nc)                                            # the last group is empty
    S, cl, cells = group_sums(sums, ncl, ok, groups, G)
    want = np.zeros((G, 6))
    for c in range(Nc):                                                            # front to back
        if ok[c]:
            want[groups[c]] += sums[c]
    assert np.array_equal(S, want) and S.dtype == np.float64
    assert np.array_equal(cl, [ncl[ok & (groups == g)].sum() for g in range(G)])
    assert np.array_equal(cells, [(ok & (groups == g)).sum() for g in range(G)]) and cells[-1] == 0
    back = np.zeros((G, 6))
    for c in reversed(range(Nc)):
        if ok[c]:
            back[groups[c]] += sums[c]
    assert not np.array_equal(back, want)                                          # the test can tell the orders apart


def test_host_iteration_over_groups_is_the_contract():
    """`solve_groups` on the checker's float64 sums lands where the checker's own iteration lands, group by group; an empty group is
    NO_DATA; max_rounds = 0 evaluates."""
    from velocycle_amd import _lib
    from velocycle_amd.cell_speed import solve_groups
    name = "bins_1025_12"
    ref = Q.group_solved(name)
    G = len(ref) + 1                                                               # and one group without a cell

    def evaluate(om):
        S, cl, cells = np.zeros((G, 6)), np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        for g, (_, _, rows) in enumerate(ref):
            at = Q.at64(name, rows, om[g])
            S[g] = [at["L"], at["score"], at["fisher"], at["observed"], at["N"], at["A"]]
            cl[g], cells[g] = at["n_clamped"], len(rows)
        return S, cl, cells

    pm, pp = np.full(G, Q.GROUP_PRIOR[0]), np.full(G, 1.0 / Q.GROUP_PRIOR[1] ** 2)
    out = solve_groups(evaluate, np.full(G, Q.START), pm, pp, 1e-10, 30)
    for g, (f64, f32, rows) in enumerate(ref):
        d = Q.omega_distance(out["omega"][g], f64)
        print(f"group {g}: {out['omega'][g]:.6f} ({d:.3g} se from the reference), {out['rounds'][g]} steps, status {out['status'][g]}")
        assert out["status"][g] in Q.INTERIOR and d <= 1e-4 and out["rounds"][g] <= f64["iterations"] and out["n_cells"][g] == len(rows)
    assert out["status"][-1] == _lib.VC_CSP_NO_DATA and out["rounds"][-1] == 0
    ev = solve_groups(evaluate, np.full(G, 0.3), pm, pp, 1e-10, 0)
    assert (ev["status"][:-1] == _lib.VC_CSP_EVALUATED).all() and (ev["omega"] == 0.3).all() and (ev["rounds"] == 0).all()
    assert (_lib.VC_CSP_CONVERGED, _lib.VC_CSP_ROUNDING, _lib.VC_CSP_MAX_ITER, _lib.VC_CSP_UNBOUNDED, _lib.VC_CSP_NO_DATA,
            _lib.VC_CSP_EVALUATED) == (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED, Q.NO_DATA, Q.EVALUATED)


def test_phase_bin_groups():
    from tests.gene_kinetics_checker import directions
    from velocycle_amd.cell_speed import phase_bin_groups
    for name in Q.GROUP_CASES:
        p = Q.cases()[name]
        bins = Q.GROUPS[name]
        want, G = Q.phase_bins(p, bins)
        got, centres = phase_bin_groups(3.0 * directions(p["phis"]), bins, p["D"])   # any length of the direction
        assert got.dtype == np.int64 and np.array_equal(got, want) and got.max() == G - 1
        assert np.allclose(centres, 2 * np.pi * (np.arange(bins) + 0.5) / bins) and centres.shape == (bins,)
    edge = np.array([[1.0, 0.0, -1.0, 0.0, 1.0], [0.0, 1.0, 0.0, -1.0, -1e-300]])    # 0, pi/2, pi, 3 pi/2 and just below 2 pi
    assert phase_bin_groups(edge, 4)[0].tolist() == [0, 1, 2, 3, 3]
    with pytest.raises(ValueError, match="one-hot"):
        phase_bin_groups(edge, 4, np.ones((2, 5)))
    with pytest.raises(ValueError, match="bins"):
        phase_bin_groups(edge, 0)
    with pytest.raises(ValueError, match="non-zero length"):
        phase_bin_groups(np.zeros((2, 3)), 4)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def csp_args(**k):
    """Arguments of vc_cell_speed with pointers that are never dereferenced: every call made with them is refused before the launch."""
    one = C.c_void_p(64)
    return [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), k.get("basis", one), k.get("K", 3),
            k.get("logm", one), k.get("nu", one), k.get("xy", one), k.get("noise", 1), k.get("r", None), k.get("prior", None),
            k.get("start", one), k.get("tol", 1e-10), k.get("max_iter", 25), k.get("omega", one), k.get("var", one), k.get("sums", one),
            k.get("dec", one), k.get("it", one), k.get("st", one), k.get("nc", one), None]


REFUSALS = [(dict(K=K), b"K must be 3 or 5") for K in (0, 1, 2, 4, 9)] + [(dict(K=7), b"H = 3")] + \
    [({name: None}, b"null") for name in ("counts", "basis", "logm", "nu", "xy", "omega", "var", "sums", "dec", "it", "st", "nc")] + \
    [(dict(start=None), b"start_dev is required"), (dict(noise=0), b"r_dev"), (dict(noise=5), b"noise must be"), (dict(Nc=0), b"Nc"),
     (dict(Ng=0), b"Ng"), (dict(Nc=1 << 31, stride=1 << 31), b"2^31"), (dict(stride=3), b"gene_stride"), (dict(max_iter=-1), b"max_iter"),
     (dict(tol=-1e-3), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(kind=7), b"count_kind")]


def test_entry_point_validates_without_a_device():
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for kw, msg in REFUSALS:
        assert lib.vc_cell_speed(*csp_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_cell_speed(*csp_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    src = open(os.path.join(ROOT, "velocycle_amd", "csrc", "vc_cell_speed.hip")).read()
    body = src[src.index('extern "C" int vc_cell_speed('):]
    launch = body.index("hipLaunchKernelGGL")
    assert 0 < body.index("gene_refuse(") < body.index("if (refused != VC_OK) return refused;") < launch
    assert body.rindex("gene_fail(") < launch < body.index("gene_launched(")
    # the header declares what the binding binds, argument for argument, and the status codes are numbered like VC_KIN_*
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    decl = re.search(r"\nint vc_cell_speed\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.EXPORTS["vc_cell_speed"][1]) == len(csp_args())
    for i, name in enumerate(("CONVERGED", "ROUNDING", "MAX_ITER", "UNBOUNDED", "NO_DATA", "EVALUATED")):
        assert f"#define VC_CSP_{name} {i}\n" in hdr and getattr(_lib, f"VC_CSP_{name}") == getattr(_lib, f"VC_KIN_{name}") == i


def test_the_kernel_has_no_scratch(tmp_path):
    """Every instantiation of vc_cell_speed_kernel reports .private_segment_fixed_size 0 in the metadata of the assembly emitted for
    gfx950 (hipcc -S --cuda-device-only), fits two workgroups of 256 lanes to a SIMD's registers, and uses 16 KiB of LDS."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "velocycle_amd", "csrc", "vc_cell_speed.hip")
    out = str(tmp_path / "csp.s")
    subprocess.run([hipcc, "-falign-loops=64", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out],
                   check=True, capture_output=True)
    txt = open(out).read()
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*vc_cell_speed_kernel\S*)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)
    assert len(found) == 8, len(found)                     # H {1, 2} x {NB, Poisson} x {u16, f32}
    print("VGPRs:", sorted({int(v) for _, _, _, v in found}))
    assert all(int(p) == 0 for _, _, p, _ in found), found
    assert all(int(lds) == 16384 and int(v) <= 256 for lds, _, _, v in found), found
    assert "global_atomic" not in txt and "ds_add" not in txt     # no atomics: every sum has its order
