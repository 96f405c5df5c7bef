"""GPU: the standard-normal stream behind every performance-mode SVI step (csrc/vc_common.h: vc_philox_normal /
vc_philox_normal2) against the float64 restatement of tests/noise_checker.py, which shares no code with it.

Every draw of every engine below: |device - normals(seed, step, global index)| <= 1e-4 (noise_checker.TOL).  The bar is a
condition, not a measurement: a wrong counter word, key word, index, cos / sin branch or site offset moves a draw by O(1), four
orders above it; float32 rounding of the same operations is 1.7e-6 (normals32) and the hardware log2 / sin / cos add their own
absolute error on a radius <= 5.9.  Each test prints the worst device error next to the worst normals32 error.

That elementwise comparison reads the draw buffer of the unfused sampler (vc_read_site(eps)): vc_philox_normal.  The fused step keeps
its draws in a ring that only vc_philox_normal2 fills and that no call reads back; the last three tests hold it through the sites the
fused kernels store (site = guide(parameters, draws), against the float64 guide on the restated draws; the bar is derived there).
Not observable through the API: the boot launch's own draw of phi_xy (csrc/vc_fused_kernels.hip, vc_tail_cell_block), which the first
step overwrites before anything can read it.
"""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import noise_checker as NC

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
STEPS = (0, 5, 1 << 31, (1 << 32) + 3, 1 << 40)


def _readable_sites(spec):
    """Every site vc_read_site serves for this model (sampled and deterministic)."""
    s = ["ν", "ϕxy", "ϕ"]
    if spec.with_delta_nu:
        s.append("Δν")
    if spec.noisemodel == "NegativeBinomial":
        s.append("shape_inv")
    if spec.kind == "velocity":
        s += ["logγg", "logβg", "νω", "ω"]
        if spec.guide == "lrmn":
            s.append("rho_real")
    return s


def _fixture_engine(case, **kw):
    from velocycle_amd.engine import HipEngine
    z = H.load_fixture(f"{H.GOLDEN}/ref_step_{case}.npz")
    spec = H.spec_from_fixture(z)
    eng = HipEngine(spec, **kw)
    eng.set_params({k[4:]: torch.tensor(v) for k, v in z.items() if k.startswith("par_")})
    return eng, spec


def _compare(eng, seed, step, label, flat=None, with32=True, ref_out=None):
    """The eps vector of the engine's last sample_guide(seed, step) against the restatement: every slot a site owns, at its global
    index.  Returns (worst device error, worst normals32 error, device draws (float64, alignment slot = nan)); the restatement's
    draws go to `ref_out` (same layout) if given."""
    names = NC.slot_names(eng)                         # (asserts: slices disjoint, cover [0, eps_total) but the alignment slot)
    owned = names != "align"
    got = (eng.read_site("eps") if flat is None else flat).double().numpy()
    assert got.shape == (eng.eps_total,)
    gidx = NC.global_index(eng)[owned]
    want = NC.normals(seed, step, gidx)
    err = np.abs(got[owned] - want)
    e32 = float(np.abs(NC.normals32(seed, step, gidx) - want).max()) if with32 else 0.0
    if ref_out is not None:
        ref_out[owned], ref_out[~owned] = want, np.nan
    if not owned.all():
        assert got[~owned].tolist() == [0.0], f"{label}: the alignment slot was written: {got[~owned]}"
    assert np.isfinite(got).all(), label
    k = int(err.argmax())
    assert err.max() <= NC.TOL, (f"{label}: step {step}: slot {np.nonzero(owned)[0][k]} (site {names[owned][k]}): "
                                 f"device {got[owned][k]!r}, restatement {want[k]!r}")
    out = got.copy()
    out[~owned] = np.nan
    return float(err.max()), e32, out


def _run_steps(eng, label, steps=STEPS, seed=SEED):
    names = NC.slot_names(eng)
    left_out = {n: int((names == n).sum()) for n in ("align",) if (names == n).any()}
    worst, worst32 = 0.0, 0.0
    for t in steps:
        eng.sample_guide(eps=None, seed=seed, step=t)
        e, e32, _ = _compare(eng, seed, t, label)
        worst, worst32 = max(worst, e), max(worst32, e32)
    cond = sorted(eng.spec.condition_on)
    print(f"\n[noise] {label}: eps_total {eng.eps_total}, sites {list(eng.eps_slices)}, conditioned sites {cond} (their slots are "
          f"drawn and compared like any other), left out by name {left_out or 'none'} = {sum(left_out.values())} of "
          f"{eng.eps_total} slots; worst |device - float64| {worst:.2e}, worst |float32 numpy - float64| {worst32:.2e}")
    # nothing but the one alignment slot is ever left out: the share of SITE slots left out is 0, conditioned fixture or not
    assert sum(left_out.values()) <= 1
    assert eng.status() == (True, -1, 0)
    return worst


@pytest.mark.parametrize("case", H.STEP_CASES)
def test_every_kernel_set_draws_the_restated_stream(case):
    eng, spec = _fixture_engine(case)
    assert not eng.stats["generic"], eng.stats
    _run_steps(eng, case)
    eng.close()


def _mean_field_velocity_case(conditioned=None):
    for case in H.STEP_CASES:
        z = H.load_fixture(f"{H.GOLDEN}/ref_step_{case}.npz")
        if z["in_kind"].item() == "velocity" and z["in_guide"].item() == "meanfield":
            if conditioned is None or conditioned == any(k.startswith("cond_") for k in z):
                return case
    raise AssertionError("no mean-field velocity fixture among tests/golden/ref_step_*.npz")


def test_run_time_sized_kernels_on_a_fast_set_configuration():
    from velocycle_amd.tuning import Tuning
    case = _mean_field_velocity_case()
    eng, spec = _fixture_engine(case, tuning=Tuning(force_generic=True))
    assert eng.stats["generic"], eng.stats
    _run_steps(eng, case + " force_generic")
    eng.close()


@pytest.mark.parametrize("kind,guide,Hw,Nx", [("phase", "meanfield", 0, 0), ("velocity", "meanfield", 1, 2), ("velocity", "lrmn", 2, 2)])
def test_configurations_that_are_generic_by_themselves(kind, guide, Hw, Nx):
    """H = 4 is outside the compiled set (tests/test_hip_sweep.py builds these): csrc/vc_generic_kernels.hip, with the LRMN guide
    also the draw of eps_W that its cell blocks repeat for themselves."""
    from tests.test_hip_sweep import _problem
    from velocycle_amd.engine import HipEngine
    p = _problem(kind, guide, "NegativeBinomial", 4, Hw, 0, Nx, [], Nc=122, Ng=11, seed=140)
    eng = HipEngine(H.spec_from_problem(p))
    assert eng.stats["generic"], eng.stats
    _run_steps(eng, f"generic H=4 {kind} {guide}")
    eng.close()


def test_shard_draws_at_its_global_indices():
    """rank 1 of 2: the ϕxy tail takes the counter of the GLOBAL cell (local index + 2 cell_offset), the replicated sites the same
    counters as rank 0 -- bit for bit."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.workloads import make_velocity_spec
    spec = make_velocity_spec(1500, 64, "vjoint")
    e0, e1 = HipEngine(spec, rank=0, world_size=2), HipEngine(spec, rank=1, world_size=2)
    for e in (e0, e1):
        e.init_params()
    assert e1.c0 == 750 and e1.eps_n_global == e0.eps_n_global
    gi = NC.global_index(e1)
    ng = e1.eps_n_global
    assert np.array_equal(gi[:ng], np.arange(ng)) and gi[ng] == ng + 2 * 750 and gi[-1] == ng + 2 * 1500 - 1
    for t in (0, (1 << 32) + 3):
        for e in (e0, e1):
            e.sample_guide(eps=None, seed=SEED, step=t)
        f0, f1 = e0.read_site("eps"), e1.read_site("eps")
        assert torch.equal(f0[:ng], f1[:ng]), "the replicated part differs between ranks"
        assert not torch.equal(f0[ng:], f1[ng:])
        _compare(e0, SEED, t, "rank 0 of 2", flat=f0)
        _compare(e1, SEED, t, "rank 1 of 2", flat=f1)
    _run_steps(e1, "rank 1 of 2 (2 x 750 cells)", steps=(5,))
    e0.close()
    e1.close()


@pytest.mark.parametrize("case", H.STEP_CASES)
def test_batched_draws_across_the_32_bit_step_boundary(case):
    """vc_sample_posterior at step0 = 2^32 - 2, five draws: draw i is the single draw of step0 + i bit for bit, whose eps are the
    restatement's at step0 + i; where ϕxy is not conditioned its batched draw is its location + the restated noise directly."""
    eng, spec = _fixture_engine(case)
    names = _readable_sites(spec)
    step0, n = (1 << 32) - 2, 5
    out = eng.sample_posterior(names, n, seed=SEED, step0=step0)
    torch.cuda.synchronize()
    locs = eng.view(eng.params, "ϕxy_locs").detach().cpu().double().numpy().reshape(-1)
    o, s = eng.eps_slices["ϕxy"]
    gxy = NC.global_index(eng)[o:o + s]
    worst, eps_by_draw = 0.0, []
    for i in range(n):
        eng.sample_guide(eps=None, seed=SEED, step=step0 + i)
        for nm in names:
            one = eng.read_site(nm)
            assert torch.equal(out[nm][i].cpu().reshape(one.shape), one), f"{case}: draw {i} site {nm}"
        e, _, flat = _compare(eng, SEED, step0 + i, f"{case} draw {i}")
        worst = max(worst, e)
        eps_by_draw.append(flat)
        if "ϕxy" not in spec.condition_on:
            want = locs + NC.normals(SEED, step0 + i, gxy)
            got = out["ϕxy"][i].cpu().double().numpy().reshape(-1)
            assert (np.abs(got - want) <= NC.TOL + 2.0 ** -23 * np.abs(want)).all(), f"{case}: draw {i}: ϕxy is not loc + eps"
    # the steps on either side of 2^32 are different streams, and step 2^32 is not step 0
    for i in range(1, n):
        assert not np.array_equal(eps_by_draw[i], eps_by_draw[i - 1], equal_nan=True)
    eng.sample_guide(eps=None, seed=SEED, step=0)
    assert not np.array_equal(eng.read_site("eps").double().numpy()[:8], np.nan_to_num(eps_by_draw[2])[:8])
    print(f"\n[noise] {case}: batched draws at steps 2^32 - 2 .. 2^32 + 2: worst |device - float64| {worst:.2e}")
    assert eng.status() == (True, -1, 0)
    eng.close()


def test_distribution_of_the_device_draws():
    """>= 2^20 device draws (8 consecutive steps of a 65536-cell phase problem, seed 20240917): N(0, 1) and independent by the
    statistics of tests/test_noise_cpu.py, bar 6.0; each statistic within 0.05 of the restatement's on the same indices."""
    from velocycle_amd.engine import HipEngine
    from velocycle_amd.workloads import make_phase_spec
    seed = 20240917
    spec = make_phase_spec(65536, 64)
    eng = HipEngine(spec)
    eng.init_params()
    assert eng.eps_total >= 1 << 17
    valid = NC.slot_names(eng) != "align"
    gidx = NC.global_index(eng)
    assert gidx[0] == 0 and np.array_equal(gidx, np.arange(eng.eps_total))
    n_steps = 8
    while n_steps * int(valid.sum()) < (1 << 20):
        n_steps += 1
    dev = {s: np.empty((n_steps, eng.eps_total)) for s in (seed, seed + 1)}
    ref = {s: np.empty((n_steps, eng.eps_total)) for s in (seed, seed + 1)}
    worst, worst32 = 0.0, 0.0
    for s in (seed, seed + 1):
        for t in range(n_steps):
            eng.sample_guide(eps=None, seed=s, step=t)
            e, e32, flat = _compare(eng, s, t, f"seed {s}", with32=(s == seed), ref_out=ref[s][t])
            worst, worst32 = max(worst, e), max(worst32, e32)
            dev[s][t] = flat
    assert eng.status() == (True, -1, 0)
    eng.close()

    def table(x):
        a, b = x[seed], x[seed + 1]
        z = NC.gof(a[:, valid])
        z["step t vs step t + 1"] = NC.cross(a[:-1][:, valid], a[1:][:, valid])
        z["seed vs seed + 1"] = NC.cross(a[:, valid], b[:, valid])
        z.update(NC.within(a, valid))
        return z

    zd, zr = table(dev), table(ref)
    n = n_steps * int(valid.sum())
    assert n >= 1 << 20
    print(f"\n[noise] {n} device draws ({n_steps} steps x {int(valid.sum())} slots): worst |device - float64| {worst:.2e}, worst "
          f"|float32 numpy - float64| {worst32:.2e} (over the same {n} indices), largest |draw| {np.nanmax(np.abs(dev[seed])):.3f}")
    print("[noise] statistic: device z | restatement z\n" + "\n".join(f"[noise]   {k:>22}: {zd[k]:+.3f} | {zr[k]:+.3f}" for k in zd))
    assert np.nanmax(np.abs(dev[seed])) <= NC.RAD_MAX + NC.TOL
    for k in zd:
        assert abs(zd[k]) <= NC.BAR, (k, zd[k])
        assert abs(zd[k] - zr[k]) <= 0.05, (k, zd[k], zr[k])


def test_rounding_edges_of_the_24_bit_uniform_on_the_device():
    """u1 = 1.0 by rounding (radius 0) and u1 = 2^-25 (the largest radius) at index 0: finite, and the restatement's value."""
    eng, spec = _fixture_engine(H.STEP_CASES[0])
    i01 = np.array([0, 1])
    for (seed, step), zero in ((NC.EDGE_ONE, True), (NC.EDGE_SMALL, False)):
        eng.sample_guide(eps=None, seed=seed, step=step)
        _, _, flat = _compare(eng, seed, step, "u1 = 1.0" if zero else "u1 = 2^-25")
        want = NC.normals(seed, step, i01)
        assert np.isfinite(flat[:2]).all()
        if zero:
            assert (np.abs(flat[:2]) <= NC.TOL).all(), flat[:2]
        else:
            assert (np.abs(flat[:2] - want) <= NC.TOL).all(), (flat[:2], want)
            assert abs(np.hypot(flat[0], flat[1]) - NC.RAD_MAX) <= 2 * NC.TOL
        print(f"\n[noise] edge {'u1 = 1.0' if zero else 'u1 = 2^-25'}: device eps[0:2] {flat[:2]}, restatement {want}")
    assert eng.status() == (True, -1, 0)
    eng.close()


# ---- the fused step: boot draws, and the eps ring that vc_philox_normal2 fills ----------------------------------------------------
# vc_read_site(eps) serves the buffer of the unfused sampler only.  The fused kernels keep their draws in a ring of their own, but they
# store every sampled site, and a site is an affine map of its draws at parameters that can be read: site = guide(params, eps).  So the
# sites read back after a fused launch are held to the float64 guide (oracle/velocycle_oracle.py: _guide) evaluated at the engine's
# parameters of that moment on the RESTATED draws.  Per element, with S = sum of the |coefficients| of the draws it takes and M = the
# sum of the magnitudes of its terms:   |device - float64| <= TOL S + 2^-19 M
# TOL S is the elementwise bar of this file carried through the map (for phi_xy, whose scale is 1, TOL itself); 2^-19 M allows 32 float32
# roundings of terms bounded by M (expf / sqrt / divide of the scales: a few ulp each; at most VC_MAX_RANK + 2 products and sums).  A draw
# from the wrong counter, index, branch or slot moves the element by O(S): the test prints the allowance in units of S and requires it
# to stay below 1e-2.
OPT = dict(lr=0.03, lrd=1.0, b1=0.8, b2=0.99, eps=1e-8, clip=10.0)
DRAWN = ("ϕxy", "ν", "logγg", "logβg", "νω")


def _expected_sites(eng, problem, seed, step):
    """{site: (float64 value, tolerance, tolerance / S)} of the guide sample at (seed, step) from the engine's CURRENT parameters."""
    spec = eng.spec
    par = {n: v.detach().cpu().double() for n, v in eng.named().items()}
    gidx = NC.global_index(eng)
    shapes = {"ν": (spec.Ng, spec.Nh), "νω": (spec.Nx, spec.Nhw), "ϕxy": (eng.Nc_local, 2)}
    eps = {k: torch.from_numpy(NC.normals(seed, step, gidx[o:o + s])).reshape(shapes.get(k, (s,))) for k, (o, s) in eng.eps_slices.items()}
    val, _ = H.orc._guide(problem, par, eps)
    c = {k: v.numpy() for k, v in H.orc.constrained(par).items()}
    a = {k: np.abs(v.numpy()) for k, v in eps.items()}
    S, M = {}, {}

    def normal_site(site, loc, scale):
        S[site], M[site] = scale + 0.0 * loc, np.abs(loc) + scale * a[site]

    normal_site("ϕxy", c["ϕxy_locs"], 1.0)
    normal_site("ν", c["ν_locs"], c["ν_scales"])
    if spec.kind == "velocity" and spec.guide == "meanfield":
        for n in ("logγg", "logβg", "νω"):
            normal_site(n, c[n + "_locs"], c[n + "_scales"])
    elif spec.kind == "velocity":
        Ng = spec.Ng
        W, D, loc = c["cov_factor"], np.sqrt(c["cov_diag"]), c["loc"]
        SX = np.abs(W).sum(1) + D
        MX = np.abs(loc) + np.abs(W) @ a["eps_W"] + D * a["eps_D"]
        S["logγg"], M["logγg"] = SX[:Ng], MX[:Ng]
        S["νω"], M["νω"] = SX[Ng:].reshape(spec.Nx, spec.Nhw), MX[Ng:].reshape(spec.Nx, spec.Nhw)
        rho = 1.998 / (1.0 + np.exp(-c["rho_real_loc"] / spec.rho_scale)) - 0.999
        k = np.abs(rho) * c["logβg_scales"] / np.sqrt((W * W).sum(1) + c["cov_diag"])[:Ng]
        sd_b = c["logβg_scales"] * np.sqrt(1.0 - rho ** 2)
        S["logβg"] = k * SX[:Ng] + sd_b
        M["logβg"] = np.abs(c["logβg_locs"]) + k * (MX[:Ng] + np.abs(loc[:Ng])) + sd_b * a["logβg"]
    out = {}
    for n in S:
        tol = NC.TOL * S[n] + 2.0 ** -19 * M[n]
        out[n] = (val[n].numpy(), tol, tol / S[n])
    return out


class _Fused:
    """One rank of a fused run: engine, optimiser state, device step counter, loss ring, exchange buffer."""

    def __init__(self, spec, step0, rank=0, world=1, params=None):
        from velocycle_amd.engine import HipEngine
        self.e = e = HipEngine(spec, rank=rank, world_size=world)
        if params is not None:
            e.set_params(params)
        else:
            cov = None
            if spec.kind == "velocity" and spec.guide == "lrmn":
                m = spec.Ng + spec.Nx * spec.Nhw
                cov = torch.normal(torch.zeros((m, spec.rho_rank)), torch.ones((m, spec.rho_rank)) * 0.02, generator=torch.Generator().manual_seed(1))
            e.init_params(cov)
        n = e.total - e.header
        self.m, self.v = torch.zeros(n, device=e.device), torch.zeros(n, device=e.device)
        self.sd = torch.full((1,), step0, dtype=torch.int64, device=e.device)
        self.ring = torch.zeros(256, dtype=torch.float64, device=e.device)
        self.x = torch.zeros(e.exchange_size(), device=e.device)
        self.problem = H.problem_from_spec(spec)
        self.worst, self.loosest, self.n_checked = {}, 0.0, 0

    def step(self, prime):
        self.e.svi_step_fused(self.m, self.v, OPT["lr"], OPT["lrd"], OPT["b1"], OPT["b2"], OPT["eps"], OPT["clip"], seed=SEED,
                              step_dev=self.sd, loss_buf=self.ring, prime=prime, n_steps=1)

    def phase(self, phase, prime=False):
        self.e.svi_run_sharded(self.x, self.m, self.v, OPT["lr"], OPT["lrd"], OPT["b1"], OPT["b2"], OPT["eps"], OPT["clip"], seed=SEED,
                               step_dev=self.sd, loss_buf=self.ring, prime=prime, phase=phase, n_steps=1)

    def check(self, step, sites, label):
        """The stored sites `sites` are the guide sample of `step` at the current parameters, on the restated draws."""
        torch.cuda.synchronize()
        want = _expected_sites(self.e, self.problem, SEED, step)
        for n in sites:
            if n not in want or n in self.e.spec.condition_on:
                continue
            w, tol, rel = want[n]
            got = self.e.read_site(n).double().numpy().reshape(w.shape)
            assert np.isfinite(got).all() and np.isfinite(w).all(), (label, n)
            err = np.abs(got - w)
            k = np.unravel_index(int((err / tol).argmax()), err.shape)
            assert (err <= tol).all(), (f"{label}: site {n} element {k} is not the guide sample of step {step} on the restated draws: "
                                        f"device {got[k]!r}, float64 {w[k]!r}, allowed {tol[k]:.2e}")
            self.worst[n] = max(self.worst.get(n, 0.0), float((err / (tol / rel)).max()))
            self.loosest = max(self.loosest, float(rel.max()))
            self.n_checked += got.size

    def report(self, label):
        spec = self.e.spec
        drawn = [n for n in DRAWN if n in _readable_sites(spec)]
        left_out = [n for n in drawn if n in spec.condition_on]
        print(f"\n[noise] {label}: {self.n_checked} site elements held to the restated draws; worst |device - float64| in units of the "
              f"element's draw coefficient S: " + ", ".join(f"{n} {v:.2e}" for n, v in self.worst.items()) +
              f"; largest allowance / S {self.loosest:.2e}; conditioned sites, whose ring slots nothing reads: {left_out or 'none'}")
        assert self.loosest <= 1e-2
        assert set(self.worst) == set(drawn) - set(left_out)
        assert self.e.status() == (True, -1, 0)


@pytest.mark.parametrize("case", H.STEP_CASES)
def test_fused_step_samples_from_the_restated_stream(case):
    """vc_svi_run_fused: the sample left behind by step k of a run is drawn from the eps ring, which only vc_philox_normal2 fills -- the
    slot of step0 + 1 by the boot launch, every later slot by the step before (three slots: four steps wrap the ring).  After each of
    four steps every sampled site is the guide sample of step0 + k at the updated parameters on the restated draws.  A second engine
    stops after the priming launches and phase A of vc_svi_run_sharded (one rank): the gene-side sites and nu_omega are then still the
    BOOT sample of step0, drawn directly (vc_philox_normal), phi_xy already the ring's sample of step0 + 1."""
    from velocycle_amd import _lib
    z = H.load_fixture(f"{H.GOLDEN}/ref_step_{case}.npz")
    spec = H.spec_from_fixture(z)
    params = {k[4:]: torch.tensor(v) for k, v in z.items() if k.startswith("par_")}
    step0 = 0
    r = _Fused(spec, step0, params=params)
    for k in range(1, 5):
        r.step(prime=(k == 1))
        r.check(step0 + k, DRAWN, f"{case} after step {k}")
        assert int(r.sd.item()) == step0 + k
    r.report(f"{case}: fused steps 1..4")
    r.e.close()
    b = _Fused(spec, step0, params=params)
    b.phase(_lib.VC_PHASE_A, prime=True)
    b.check(step0, ("ν", "logγg", "logβg", "νω"), f"{case} boot sample")
    b.check(step0 + 1, ("ϕxy",), f"{case} after phase A")
    b.report(f"{case}: boot + phase A")
    b.e.close()


def test_fused_step_ring_across_the_32_bit_step_boundary():
    """The same from step0 = 2^32 - 2: the ring slots of steps 2^32 - 1 .. 2^32 + 2 (`s + 1` of the launch that fills them) take all 64
    bits of the step."""
    spec = H.spec_from_fixture(H.load_fixture(f"{H.GOLDEN}/ref_step_{_mean_field_velocity_case(conditioned=False)}.npz"))
    assert not spec.condition_on
    step0 = (1 << 32) - 2
    r = _Fused(spec, step0)
    for k in range(1, 5):
        r.step(prime=(k == 1))
        r.check(step0 + k, DRAWN, f"step {step0} + {k}")
    assert int(r.sd.item()) == step0 + 4
    r.report("fused steps 2^32 - 1 .. 2^32 + 2")
    r.e.close()


def test_sharded_fused_step_samples_at_global_indices():
    """vc_svi_run_sharded on ranks 0 and 1 of 2 (750 cells each; the test adds the two exchange buffers as the all-reduce would): the
    ring of rank 1 holds phi_xy at the counters of the GLOBAL cells (pair + cell_offset) and the replicated sites at the same counters
    as rank 0.  After the priming launches + phase A (boot sample of the gene side, ring sample of phi_xy) and after each of three
    whole steps every sampled site of both ranks is the guide sample on the restated draws; the replicated sites agree bit for bit."""
    from velocycle_amd import _lib
    from velocycle_amd.workloads import make_velocity_spec
    spec = make_velocity_spec(1500, 64, "vjoint")
    step0 = 3
    ranks = [_Fused(spec, step0, rank=q, world=2) for q in range(2)]
    assert ranks[1].e.c0 == 750
    for k in range(1, 4):
        for q, r in enumerate(ranks):
            r.phase(_lib.VC_PHASE_A, prime=(k == 1))
            if k == 1:
                r.check(step0, ("ν", "logγg", "logβg", "νω"), f"rank {q} of 2, boot sample")
                r.check(step0 + 1, ("ϕxy",), f"rank {q} of 2, after phase A")
        torch.cuda.synchronize()
        tot = ranks[0].x + ranks[1].x
        for q, r in enumerate(ranks):
            r.x.copy_(tot)
            r.phase(_lib.VC_PHASE_B)
            r.check(step0 + k, DRAWN, f"rank {q} of 2 after step {k}")
        for n in ("ν", "logγg", "logβg", "νω"):
            assert torch.equal(ranks[0].e.read_site(n), ranks[1].e.read_site(n)), f"step {k}: replicated site {n} differs between ranks"
        assert not torch.equal(ranks[0].e.read_site("ϕxy"), ranks[1].e.read_site("ϕxy"))
    for q, r in enumerate(ranks):
        r.report(f"rank {q} of 2 (2 x 750 cells), steps {step0 + 1}..{step0 + 3}")
        r.e.close()
