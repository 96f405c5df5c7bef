"""CPU: the float64 checker of the maximum-likelihood phase assignment (tests/mle_checker.py) against the stored output of the
reference's own Phases.from_cycle_mle (tests/golden/ref_cycle_mle_*.npz, written by tests/golden/make_golden_mle.py); the public
face (signature, refusals before any device work); the C ABI declaration and its binding."""
import glob
import inspect
import os
import re
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import torch

from tests import mle_checker as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(os.path.basename(p)[len("ref_cycle_mle_"):-4] for p in glob.glob(os.path.join(GOLDEN, "ref_cycle_mle_*.npz")))
EXCUSED_CAP = 0.05


def load(case):
    z = np.load(os.path.join(GOLDEN, f"ref_cycle_mle_{case}.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def regret_bar():
    """4 x the float32 reference's own worst regret ratio over the fixtures."""
    return MC.SAFETY * np.nanmax([float(load(c)["ref_regret_ratio"]) for c in CASES])


def profile_bar():
    return MC.SAFETY * np.nanmax([float(load(c)["ref_profile_err"]) for c in CASES])


@lru_cache(maxsize=None)
def checked(case):
    z = load(case)
    T = MC.table64(z["means"], int(z["bins"]))
    logP, absP = MC.logp64(z["counts"], T, z["n_scounts"], float(z["a"]), str(z["noisemodel"]), z["dispersion"])
    return z, logP, absP


def assert_judged(case, chosen, bar=None):
    """The rules of a result: regret for every cell; on the 100-bin cases the float64 bin and the reference's wherever the
    float64 top-two margin is at least 8 eps32 A_c."""
    z, logP, absP = checked(case)
    j = MC.judge(logP, absP, chosen)
    bar = regret_bar() if bar is None else bar
    print(f"{case}: worst regret ratio {j['regret_ratio'].max():.3f} (bar {bar:.3f}), bins differing from float64 "
          f"{int((np.asarray(chosen) != j['best']).sum())}, excused share {j['excused'].mean():.4f}")
    assert j["regret_ratio"].max() <= bar, (case, j["regret_ratio"].max(), bar)
    if int(z["bins"]) == 100:
        clear = ~j["excused"]
        assert (np.asarray(chosen)[clear] == j["best"][clear]).all(), case
        assert (np.asarray(chosen)[clear] == z["ref_bin"][clear]).all(), case
    return j


def test_fixtures_present():
    assert {"a_poisson", "a_nb", "b_nb_360", "c_wide_nb", "c_wide_poisson", "d_h2_disp"} <= set(CASES)
    for c in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_cycle_mle_{c}.npz")) < (1 << 20)


@pytest.mark.parametrize("case", ["a_poisson", "a_nb", "c_wide_nb", "c_wide_poisson", "d_h2_disp", "b_nb_360"])
def test_checker_against_stored_reference(case):
    z, logP, absP = checked(case)
    j = assert_judged(case, z["ref_bin"])
    # the stored caps and measurements hold on what is committed
    assert abs(float(j["excused"].mean()) - float(z["excused_share"])) < 1e-12
    if int(z["bins"]) == 100:
        assert float(z["excused_share"]) <= EXCUSED_CAP
    if np.isfinite(z["ref_regret_ratio"]):
        assert abs(j["regret_ratio"].max() - float(z["ref_regret_ratio"])) <= 1e-6 * max(1.0, float(z["ref_regret_ratio"]))
    # the stored phi_xy is 10 (cos, sin) of the stored bin's phase
    ph = MC.grid_phases(int(z["bins"]))[torch.as_tensor(z["ref_bin"])]
    assert np.allclose(z["ref_phi_xy"], 10.0 * torch.stack([torch.cos(ph), torch.sin(ph)]).numpy(), atol=1e-5)


def test_bars_come_from_the_reference():
    assert 0 < regret_bar() < 64 and 0 < profile_bar() < 64


def test_signature_is_the_reference_s():
    from velocycle_amd.containers import Phases
    sig = inspect.signature(Phases.from_cycle_mle)
    pos = [(n, p.default) for n, p in sig.parameters.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert pos == [("self", inspect.Parameter.empty), ("cycle", inspect.Parameter.empty), ("data", inspect.Parameter.empty), ("a", 1),
                   ("bins", 100), ("concentration", 10.), ("noisemodel", "Poisson"), ("dispersion", 0.3)]
    kw = {n: p.default for n, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY}
    assert kw == {"device": None, "chunk_cells": None, "return_profile": False}


def _objects(Nc=5, Ng=4):
    from velocycle_amd.anndata_lite import AnnDataLite
    from velocycle_amd.containers import Cycle, Phases
    S = np.arange(Nc * Ng, dtype=np.float32).reshape(Nc, Ng) + 1
    ad = AnnDataLite(S, S, obs=pd.DataFrame({"n_scounts": S.sum(1)}, index=[f"c{i}" for i in range(Nc)]))
    cyc = Cycle.from_array(np.zeros((3, Ng)), np.ones((3, Ng)), gene_names=list(ad.var.index))
    return ad, cyc, Phases.flat_prior(ad)


def test_refusals_fire_before_the_device(monkeypatch):
    from velocycle_amd import _lib, phase_mle
    from velocycle_amd.containers import Cycle

    def no_device(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    ad, cyc, ph = _objects()
    with pytest.raises(NotImplementedError, match="Not implemented yet, sorry"):
        ph.from_cycle_mle(cyc, ad, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="bins"):
        ph.from_cycle_mle(cyc, ad, bins=0)
    other = Cycle.from_array(np.zeros((3, 4)), np.ones((3, 4)), gene_names=["x", "y", "z", "w"])
    with pytest.raises(ValueError, match="genes"):
        ph.from_cycle_mle(other, ad)
    fewer = Cycle.from_array(np.zeros((3, 3)), np.ones((3, 3)), gene_names=list(ad.var.index)[:3])
    with pytest.raises(ValueError, match="genes"):
        ph.from_cycle_mle(fewer, ad)
    ad.obs.loc[ad.obs.index[2], "n_scounts"] = 0.0
    with pytest.raises(ValueError, match="n_scounts"):
        ph.from_cycle_mle(cyc, ad)
    ad, cyc, ph = _objects()
    with pytest.raises(ValueError, match="dispersion"):
        ph.from_cycle_mle(cyc, ad, noisemodel="NegativeBinomial", dispersion=0.0)
    with pytest.raises(ValueError, match="dispersion"):
        ph.from_cycle_mle(cyc, ad, noisemodel="NegativeBinomial", dispersion=np.array([0.3, 0.3, -1.0, 0.3]))
    # the worker refuses the same by itself
    T, m, S = np.zeros((2, 4)), np.ones(5), np.ones((5, 4), dtype=np.float32)
    with pytest.raises(NotImplementedError):
        phase_mle.phase_mle(S, T, m, noisemodel="Lognormal")
    with pytest.raises(ValueError, match="bins"):
        phase_mle.phase_mle(S, np.zeros((0, 4)), m)
    with pytest.raises(ValueError, match="bins"):
        phase_mle.phase_mle(S, np.zeros((phase_mle.MAX_BINS + 1, 4)), m)
    with pytest.raises(ValueError, match="count factor"):
        phase_mle.phase_mle(S, T, np.array([1, 1, 0, 1, 1.0]))
    with pytest.raises(ValueError, match="dispersion"):
        phase_mle.phase_mle(S, T, m, noisemodel="NegativeBinomial", dispersion=-0.3)
    assert ph.phi_xy.values.any() == False                                 # noqa: E712  (nothing was assigned)


def test_header_declares_and_lib_binds_vc_phase_mle():
    from velocycle_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "velocycle_hip.h")).read()
    assert re.search(r"\bint vc_phase_mle\(const void\* counts_dev, int count_kind", hdr)
    assert "phases.py:471-509" in hdr and "#define VC_ABI_VERSION 2" in hdr
    assert "vc_phase_mle" in _lib.EXPORTS and len(_lib.EXPORTS["vc_phase_mle"][1]) == 14
    assert (_lib.VC_COUNTS_F32, _lib.VC_COUNTS_U16) == (0, 1)


def test_entry_point_validates_without_a_device():
    import ctypes as C
    from velocycle_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    one = C.c_void_p(64)                    # never dereferenced: every call below is refused before the launch
    args = lambda **k: [k.get("counts", one), k.get("kind", 0), k.get("Ng", 4), k.get("Nc", 4), k.get("stride", 4), one, one,      # noqa: E731
                        k.get("bins", 10), one, k.get("noise", 1), k.get("r", None), one, None, None]
    assert lib.vc_phase_mle(*args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    assert b"Lognormal" in lib.vc_last_error(None)
    assert lib.vc_phase_mle(*args(bins=0)) == _lib.VC_ERR_ARG
    assert lib.vc_phase_mle(*args(bins=5000)) == _lib.VC_ERR_ARG and b"bins" in lib.vc_last_error(None)
    assert lib.vc_phase_mle(*args(Ng=0)) == _lib.VC_ERR_ARG
    assert lib.vc_phase_mle(*args(stride=3)) == _lib.VC_ERR_ARG
    assert lib.vc_phase_mle(*args(kind=7)) == _lib.VC_ERR_ARG
    assert lib.vc_phase_mle(*args(counts=None)) == _lib.VC_ERR_ARG
    assert lib.vc_phase_mle(*args(noise=0)) == _lib.VC_ERR_ARG and b"r_dev" in lib.vc_last_error(None)


def test_default_chunk_stays_under_the_stated_bound():
    from velocycle_amd import phase_mle
    for Ng in (1, 7, 200, 2000, 30000):
        n = phase_mle.default_chunk_cells(Ng)
        assert n >= 64 and n % 64 == 0 and (n == 64 or 4 * Ng * n <= phase_mle.CHUNK_BYTES)
