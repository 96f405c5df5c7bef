"""GPU: Phases.from_cycle_mle / velocycle_amd.phase_mle on the HIP kernel vc_phase_mle, judged by the float64 checker
(tests/mle_checker.py) with bars that come from the float32 reference's own error on the fixtures (tests/test_cycle_mle_cpu.py)."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import mle_checker as MC
from tests import test_cycle_mle_cpu as F
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.phase_mle import default_chunk_cells, phase_mle
from velocycle_amd.simulate import simulate_counts
from velocycle_amd.utils import circular_corrcoef

pytestmark = pytest.mark.gpu
ALL = ["a_poisson", "a_nb", "b_nb_360", "c_wide_nb", "c_wide_poisson", "d_h2_disp"]


def objects(z, sparse=False):
    S = z["counts"].astype(np.float32)
    layer = sp.csr_matrix(S) if sparse else S
    ad = AnnDataLite(layer, layer, obs=pd.DataFrame({"n_scounts": z["n_scounts"]}, index=[f"c{i}" for i in range(S.shape[0])]))
    cyc = Cycle.from_array(z["means"], np.ones_like(z["means"]), gene_names=list(ad.var.index))
    return ad, cyc, Phases.flat_prior(ad)


def run(z, sparse=False, **kw):
    ad, cyc, ph = objects(z, sparse)
    disp = z["dispersion"] if z["dispersion"].ndim else float(z["dispersion"])
    out = ph.from_cycle_mle(cyc, ad, a=float(z["a"]), bins=int(z["bins"]), noisemodel=str(z["noisemodel"]), dispersion=disp, **kw)
    return ph, out


@pytest.mark.parametrize("case", ALL)
def test_fixture_through_the_public_method(case):
    z, logP, absP = F.checked(case)
    ph, out = run(z, return_profile=True)
    best, prof = out[0].cpu().numpy(), out[1].cpu().double()
    j = F.assert_judged(case, best)
    # in-place effect: 10 (cos, sin) of the chosen phase, like the reference
    phis = MC.grid_phases(int(z["bins"]))[torch.as_tensor(best)]
    assert np.array_equal(ph.phi_xy.values.astype(np.float32), (10. * torch.stack([torch.cos(phis), torch.sin(phis)])).numpy())
    same = best == z["ref_bin"]
    assert np.array_equal(ph.phi_xy.values.astype(np.float32)[:, same], z["ref_phi_xy"][:, same])
    # profile: <= 0, exactly 0 at the chosen bin, within 4 x the float32 reference's own error of the float64 profile
    cols = torch.arange(prof.shape[1])
    assert float(prof.max()) == 0.0 and bool((prof[torch.as_tensor(best), cols] == 0).all())
    err = ((prof - MC.profile64(logP)).abs() / (MC.EPS32 * torch.as_tensor(j["A"]))).max().item()
    print(f"{case}: profile error {err:.3f} eps32 A_c (bar {F.profile_bar():.3f})")
    assert err <= F.profile_bar(), (case, err)
    # None like the reference without return_profile; a CSR layer gives the same bits
    ph2, out2 = run(z, sparse=True)
    assert out2 is None and np.array_equal(ph2.phi_xy.values, ph.phi_xy.values)


def problem(Nc, Ng, bins, seed=0, noise="NegativeBinomial"):
    sim = simulate_counts(Nc=max(Nc, 2), Ng=Ng, seed=seed)
    S = sim["S"][:Nc].numpy()
    n = np.maximum(S.sum(1), 1.0).astype(np.float64)
    means = sim["nu"].numpy().T.astype(np.float64).copy()
    means[0] -= np.log(n.mean())
    return S, MC.table64(means, bins), n


@pytest.mark.parametrize("Nc,Ng,bins", [(1, 7, 33), (63, 1, 2), (65, 257, 100), (1000, 7, 1000), (65, 7, 1), (63, 257, 33), (1000, 257, 100)])
@pytest.mark.parametrize("noise", ["NegativeBinomial", "Poisson"])
def test_ragged_shapes(Nc, Ng, bins, noise):
    S, T, n = problem(Nc, Ng, bins, seed=Nc + Ng)
    best, prof = phase_mle(S, T, n, noisemodel=noise, dispersion=0.3, return_profile=True)
    logP, absP = MC.logp64(S, T, n, 1.0, noise, 0.3)
    j = MC.judge(logP, absP, best.cpu().numpy())
    assert j["regret_ratio"].max() <= F.regret_bar(), j["regret_ratio"].max()
    assert tuple(prof.shape) == (bins, Nc) and float(prof.max()) == 0.0
    err = ((prof.cpu().double() - MC.profile64(logP)).abs() / (MC.EPS32 * torch.as_tensor(j["A"]))).max().item()
    assert err <= F.profile_bar(), err
    # storage: uint16 and float32 give identical bits
    b32, p32 = phase_mle(S, T, n, noisemodel=noise, dispersion=0.3, return_profile=True, storage="f32")
    assert torch.equal(b32, best) and torch.equal(p32, prof)


def test_large_count_zero_gene_zero_cell():
    S, T, n = problem(130, 40, 100, seed=5)
    S[3, 2] = 70000.0             # forces float32 storage
    S[:, 7] = 0.0                 # a gene nobody expresses
    S[11, :] = 0.0                # a cell without counts whose n_scounts stays > 0
    for noise in ("NegativeBinomial", "Poisson"):
        best, prof = phase_mle(S, T, n, noisemodel=noise, dispersion=0.3, return_profile=True)
        logP, absP = MC.logp64(S, T, n, 1.0, noise, 0.3)
        j = MC.judge(logP, absP, best.cpu().numpy())
        assert j["regret_ratio"].max() <= F.regret_bar(), (noise, j["regret_ratio"].max())
        assert bool(torch.isfinite(prof).all())
        with pytest.raises(ValueError, match="65535"):
            phase_mle(S, T, n, noisemodel=noise, storage="u16")


def test_planted_ties_take_the_lower_bin():
    bins = 100
    S, T, n = problem(300, 33, bins, seed=9)
    T = T.clone()
    T[bins // 2:] = T[:bins // 2]                     # bins j and j + bins / 2 are the same row: equal likelihoods, bit for bit
    for noise in ("NegativeBinomial", "Poisson"):
        best, prof = phase_mle(S, T, n, noisemodel=noise, return_profile=True)
        assert int(best.max()) < bins // 2
        assert torch.equal(prof[:bins // 2], prof[bins // 2:])


def test_deterministic_and_independent_of_the_chunk_size():
    z = F.load("a_nb")
    T = MC.table64(z["means"], int(z["bins"]))
    S = z["counts"].astype(np.float32)
    outs = [phase_mle(S, T, z["n_scounts"], noisemodel="NegativeBinomial", dispersion=0.3, return_profile=True, chunk_cells=c)
            for c in (None, None, 64, 1000, S.shape[0])]
    for b, p in outs[1:]:
        assert torch.equal(b, outs[0][0]) and torch.equal(p, outs[0][1])
    csr = phase_mle(sp.csr_matrix(S), T, z["n_scounts"], noisemodel="NegativeBinomial", dispersion=0.3, return_profile=True, chunk_cells=1000)
    assert torch.equal(csr[0], outs[0][0]) and torch.equal(csr[1], outs[0][1])


def test_full_size_without_a_bins_genes_cells_tensor():
    Nc, Ng, bins = 50_000, 2_000, 100
    dev = torch.device("cuda")
    sim = simulate_counts(Nc=Nc, Ng=Ng, seed=21, device=dev)
    S = sim["S"]
    del sim["U"]
    n = S.sum(1).clamp_min(1.0).double().cpu()
    means = sim["nu"].T.double().cpu().clone()
    means[0] -= torch.log(n.mean())
    T = MC.table64(means.numpy(), bins)
    disp = sim["shape_inv"].double().cpu().clamp_min(0.05).numpy()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    best, prof = phase_mle(S, T, n, noisemodel="NegativeBinomial", dispersion=disp, return_profile=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    chunk = 4 * Ng * min(Nc, default_chunk_cells(Ng))
    outputs = (4 + 8) * Nc + 2 * 4 * bins * Nc
    # the counts are there already (`before`); a chunk's block and its conversions (float32 source, transposed copy, int32, mask,
    # int16: < 4 blocks), the outputs, the tables.  One [bins][Ng][Nc] float32 tensor would be 40 GB.
    assert peak <= 4 * chunk + outputs + (64 << 20), (peak, chunk, outputs)
    assert peak < 4 * bins * Ng * Nc / 16
    idx = torch.randperm(Nc, generator=torch.Generator().manual_seed(0))[:512]
    Ssub = S[idx.to(dev)].cpu().numpy()
    logP, absP = MC.logp64(Ssub, T, n[idx].numpy(), 1.0, "NegativeBinomial", disp)
    j = MC.judge(logP, absP, best[idx.to(dev)].cpu().numpy())
    # The bar: 4 x the largest ratio the float32 reference reaches on the fixtures.  (The reference agrees with float64 in every
    # cell of the wide fixtures (C), whose own stored ratio is therefore 0 and gives no bar of its own.)
    print(f"full size: worst regret ratio {j['regret_ratio'].max():.3f} (bar {F.regret_bar():.3f})")
    assert j["regret_ratio"].max() <= F.regret_bar(), j["regret_ratio"].max()
    clear = ~j["excused"]
    assert (best[idx.to(dev)].cpu().numpy()[clear] == j["best"][clear]).all()
    err = ((prof[:, idx.to(dev)].cpu().double() - MC.profile64(logP)).abs() / (MC.EPS32 * torch.as_tensor(j["A"]))).max().item()
    assert err <= F.profile_bar(), err


def test_end_to_end_recovers_the_simulated_phases():
    sim = simulate_counts(Nc=3000, Ng=200, seed=3)
    S = sim["S"].numpy()
    n = S.sum(1).astype(np.float64)
    means = sim["nu"].numpy().T.astype(np.float64).copy()
    means[0] -= np.log(n.mean())
    ad = AnnDataLite(S, S, obs=pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(len(n))]))
    cyc = Cycle.from_array(means, np.ones_like(means), gene_names=list(ad.var.index))
    cyc.set_disp_pyro(sim["shape_inv"].numpy())
    ph = Phases.flat_prior(ad)
    ph.from_cycle_mle(cyc, ad, noisemodel="NegativeBinomial", dispersion=np.maximum(cyc.disp_pyro, 0.05))
    logP, _ = MC.logp64(S, MC.table64(means, 100), n, 1.0, "NegativeBinomial", np.maximum(cyc.disp_pyro, 0.05))
    want = circular_corrcoef(MC.grid_phases(100)[torch.argmax(logP, 0)].numpy(), sim["phis"].numpy())
    got = circular_corrcoef(ph.phis.numpy(), sim["phis"].numpy())
    print(f"end to end: circular correlation with the true phases {got:.4f} (float64 assignment: {want:.4f})")
    assert want > 0.5 and got >= want - 0.01
