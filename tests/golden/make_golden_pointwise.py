#!/usr/bin/env python
"""Golden fixtures of the pointwise predictive density: tests/golden/ref_pointwise_<case>.npz.

Runs the REFERENCE's own model functions (phase_latent_variable_model, velocity_latent_variable_model[_LRMN]), unmodified, through
oracle.ref_loader (build container only): for every draw the model is conditioned on that draw's site values, run under the trace,
and the per-element log_prob of the observed sites "S" / "U" is taken.  The draws come from the oracle's guide at perturbed
parameters, so that the spread over draws is not degenerate.  What is written is DATA: the inputs (`in_*` / `cond_*`, the keys
tests/helpers reads), the draws (`draw_<site>`, float32), the reference's reduced results in float64 (`ref_<M>_<quantity>_gene |
_cell`) and, per quantity, the worst error ratio of the reference run in FLOAT32 against the float64 checker
(tests/pointwise_checker.py): ref_err_lppd, ref_err_mean, ref_err_pwaic.
The script ABORTS unless the float64 checker and the float64 reference agree within 1e-10 of the scale A on every element and sum,
and unless the float32 reference is finite and within a ratio of 64 on every case.

Usage:  python tests/golden/make_golden_pointwise.py [--check] [<case> ...]
  --check   write nothing: regenerate in memory and compare with the committed files (exit status 1 on any difference)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))

_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(OUT, "make_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)                            # loads the reference (oracle.ref_loader) and builds inputs with its containers
vc, pyro, orc = MG.vc, MG.pyro, MG.orc
from tests import pointwise_checker as PC              # noqa: E402

AGREE = 1e-10
# name: the case dict of make_golden.make_case + D draws; `big`: a gene scaled past 255 counts; gene 0 is set to zero everywhere
CASES = {
    "phase_nb": dict(kind="phase", Nc=400, Ng=60, H=1, nb=1, noise="NegativeBinomial", wdn=False, D=12),
    "phase_poisson": dict(kind="phase", Nc=300, Ng=40, H=1, nb=1, noise="Poisson", wdn=False, D=8),
    "vel_mf_joint_nb": dict(kind="velocity", Nc=500, Ng=80, H=1, Hw=1, nb=1, noise="NegativeBinomial", model_type="normal", wdn=False, D=10),
    "vel_lrmn_cond": dict(kind="velocity", Nc=600, Ng=100, H=1, Hw=1, nb=1, noise="NegativeBinomial", model_type="lrmn", wdn=False,
                          cond=["ϕxy", "ν", "shape_inv"], D=16),
    "vel_mf_dnu2": dict(kind="velocity", Nc=300, Ng=40, H=1, Hw=1, nb=2, noise="NegativeBinomial", model_type="normal", wdn=True, D=8),
    "phase_h2_poisson": dict(kind="phase", Nc=700, Ng=300, H=2, nb=1, noise="Poisson", wdn=False, D=8),
}
BIG_GENE, BIG_SCALE = 1, 40.0


def metaparams(c, seed):
    d, ad, cyc, ph, Db = MG.build_inputs(c["Nc"], c["Ng"], c["H"], c["nb"], seed)
    # a gene of zeros and a gene with counts above 255 (its constant harmonic moves with it)
    for layer in ("spliced", "unspliced"):
        M = ad.layers[layer]
        M[:, 0] = 0
        M[:, BIG_GENE] = np.round(M[:, BIG_GENE] * BIG_SCALE + 3)
    means = cyc.means.values.copy()
    means[0, BIG_GENE] += np.log(BIG_SCALE)
    means[0, 0] = -3.0
    cyc.set_means(means)
    rs = np.random.RandomState(seed + 1)
    Nc, cond = ad.n_obs, {}
    if c["kind"] == "phase":
        mp = vc.preprocessing.preprocess_for_phase_estimation(ad, cyc, ph, Db, n_harmonics=c["H"], noisemodel=c["noise"],
                                                              with_delta_nu=c["wdn"])
    else:
        spd = vc.angularspeed.AngularSpeed.trivial_prior(condition_names=[f"b{i}" for i in range(c["nb"])], harmonics=c["Hw"])
        if c["Hw"] == 1:
            spd.stds.loc["nu1_cos"] = [0.05] * c["nb"]
            spd.stds.loc["nu1_sin"] = [0.05] * c["nb"]
        S = ad.layers["spliced"]
        cf = torch.tensor(np.log(S.sum(1) / S.sum(1).mean())).float()[None, None, :]
        for site in c.get("cond", []):
            if site == "ϕxy":
                cond[site] = ph.phi_xy_tensor.T + torch.tensor(0.05 * rs.randn(Nc, 2)).float()
            elif site == "ν":
                cond[site] = cyc.means_tensor.T.unsqueeze(-2) + torch.tensor(0.05 * rs.randn(c["Ng"], 1, 2 * c["H"] + 1)).float()
            elif site == "shape_inv":
                cond[site] = torch.tensor(rs.uniform(0.2, 1.0, (c["Ng"], 1))).float()
        mp = vc.preprocessing.preprocess_for_velocity_estimation(
            ad, cyc, ph, spd, Db.float(), Db.float(), n_harmonics=c["H"], ω_n_harmonics=c["Hw"], count_factor=cf,
            noisemodel=c["noise"], with_delta_nu=c["wdn"], condition_on=cond, model_type=c.get("model_type", "lrmn"))
    return mp, cond


def draw_sites(p32, D, seed):
    """D draws of the oracle's guide at perturbed parameters (conditioned sites keep their values): {site: (D, *canonical shape)}."""
    gen = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed + 2)
    first = orc.draw_eps(p32, gen)
    par = orc.init_params(p32, first.get("_cov_factor_draw"))
    par["ν_locs"] = par["ν_locs"] + torch.tensor(0.05 * rs.randn(*par["ν_locs"].shape)).float()
    par["ν_scales"] = torch.full_like(par["ν_scales"], float(np.log(0.03)))
    par["ϕxy_locs"] = 3.0 * par["ϕxy_locs"]                       # |locs| = 6 against the unit draw noise: phases spread by ~0.17 rad
    if "shape_inv_locs" in par:
        par["shape_inv_locs"] = torch.tensor(np.log(rs.uniform(0.2, 1.0, par["shape_inv_locs"].shape))).float()
    if "Δν_locs" in par:
        par["Δν_locs"] = torch.tensor(0.1 * rs.randn(*par["Δν_locs"].shape)).float()
    out = {}
    for _ in range(D):
        val, _ = orc._guide(p32, par, orc.draw_eps(p32, gen))
        for name in p32.condition_on:
            val[name] = p32.cond(name)
        for k, v in val.items():
            if k in PC.SITES or k == "rho_real":
                out.setdefault(k, []).append(v.detach().float())
    return {k: torch.stack(v) for k, v in out.items()}


def pyro_shape(kind, name, v):
    """canonical site value -> the shape the reference's model samples it in"""
    if name == "ν":
        return v.unsqueeze(-2)
    if name == "ϕxy":
        return v
    if name == "νω":
        return v[:, :, None, None]
    if name == "Δν":
        return v[:, :, None] if kind == "phase" else v[:, None, None, :, None]
    return v.unsqueeze(-1)


def reference_log_probs(mp, kind, draws, dtype):
    """{matrix: (D, Ng, Nc)}: log_prob of the observed sites of the reference's model, one traced run per draw."""
    conv = lambda t: t.to(dtype) if (torch.is_tensor(t) and t.is_floating_point()) else t
    mpd = mp._replace(**{f: conv(getattr(mp, f)) for f in mp._fields})
    D = draws["ν"].shape[0]
    out = {}
    for i in range(D):
        data = {k: pyro_shape(kind, k, v[i].to(dtype)) for k, v in draws.items()}
        tr = pyro.poutine.trace(pyro.poutine.condition(mpd.model_fn, data=data)).get_trace(mpd)
        for m in ("S", "U"):
            if m in tr.nodes:
                lp = tr.nodes[m]["log_prob"] if "log_prob" in tr.nodes[m] else tr.nodes[m]["fn"].log_prob(tr.nodes[m]["value"])
                assert tr.nodes[m]["is_observed"] and lp.dtype == dtype, (m, lp.dtype)
                out.setdefault(m, []).append(lp.detach().reshape(int(mp.Ng), int(mp.Nc)))
    return {m: torch.stack(v) for m, v in out.items()}


def reduced(lp):
    dense = {}
    for m, l in lp.items():
        a, b, c = PC.reduce_draws(l)
        dense[m] = {"lppd": a, "mean": b, "pwaic": c}
    return dense


def generate(name, seed=21):
    c = CASES[name]
    mp, cond = metaparams(c, seed)
    p32 = orc.problem_from_metaparams(mp, c["kind"], cond, dtype=torch.float64).to(torch.float32)
    S = p32.S.numpy()
    assert S.max() > 255 and (S[0] == 0).all(), (S.max(), S[0].max())
    draws = draw_sites(p32, c["D"], seed)
    z = MG.problem_arrays(p32)
    for k, v in draws.items():
        if k in PC.SITES:
            same = bool((v == v[:1]).all())
            z["draw_" + k] = (v[:1] if same else v).numpy()
    e64 = PC.evaluate(z)
    ref64 = reduced(reference_log_probs(mp, c["kind"], draws, torch.float64))
    agree = PC.ratios(PC.as_got(ref64), e64)
    worst = max(agree.values()) * PC.EPS32          # in units of A
    ref32 = reduced({m: v.double() for m, v in reference_log_probs(mp, c["kind"], draws, torch.float32).items()})
    r32 = PC.ratios(PC.as_got(ref32), e64)
    spread = {m: float(torch.sqrt(e64[m]["pwaic"]).median()) for m in e64}
    print(f"{name}: checker vs float64 reference {worst:.2e} A; float32 reference ratios " +
          ", ".join(f"{q} {r32[q]:.3f}" for q in PC.QUANT) + f"; median sd over draws {spread}")
    assert worst <= AGREE, f"{name}: the float64 checker disagrees with the float64 reference: {worst:.3e} A"
    assert all(np.isfinite(v) and 0 < v < PC.SANITY for v in r32.values()), f"{name}: float32 reference outside the sanity band: {r32}"
    s64 = PC.sums(ref64)
    for m in s64:
        for q in PC.QUANT:
            z[f"ref_{m}_{q}_gene"] = s64[m][q]["gene"].numpy()
            z[f"ref_{m}_{q}_cell"] = s64[m][q]["cell"].numpy()
    for q in PC.QUANT:
        z["ref_err_" + q] = np.float64(r32[q])
    z["n_draws"] = np.int64(c["D"])
    return z


def main(argv):
    check = "--check" in argv
    names = [a for a in argv if not a.startswith("--")] or list(CASES)
    bad = 0
    for name in names:
        z = generate(name)
        path = os.path.join(OUT, f"ref_pointwise_{name}.npz")
        if check:
            old = np.load(path, allow_pickle=False)
            for k, v in z.items():
                v = np.asarray(v)
                same = k in old.files and v.shape == old[k].shape and (
                    np.allclose(v, old[k], rtol=1e-6, atol=1e-6, equal_nan=True) if v.dtype.kind == "f" else np.array_equal(v, old[k]))
                if not same:
                    print(f"  MISMATCH {name}:{k}")
                    bad += 1
        else:
            np.savez_compressed(path, **z)
            print("  wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
