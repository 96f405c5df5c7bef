"""GPU: the five engine-less entry points of include/velocycle_hip.h -- vc_gene_glm, vc_gene_glm_batch, vc_gene_dispersion,
vc_gene_kinetics, vc_phase_mle -- called directly in every layout their header allows (tests/cabi_layouts.py; what the layouts are is
checked without a device in tests/test_cabi_layouts_cpu.py).  The six later entry points: tests/test_hip_cabi_layouts_six.py.

Anchor: the `compact` direct call (gene_stride == Nc, the workers' convention) is held to the float64 checker at the standing bars of
that kernel's own GPU test file, through that file's judging helper, and equals the Python worker bit for bit on every output the worker
hands through.  Every other layout must then equal `compact` on every output, byte for byte, with both guard bands of every output
intact.  No tolerance of its own anywhere in this file."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import cabi_layouts as L
from tests import gene_batch_checker as BC
from tests import gene_dispersion_checker as D
from tests import gene_glm_checker as G
from tests import gene_kinetics_checker as Q
from tests import mle_checker as MC
from tests import test_cycle_mle_cpu as F
from tests import test_hip_cycle_mle as TM
from tests import test_hip_gene_batch as TB
from tests import test_hip_gene_dispersion as TD
from tests import test_hip_gene_harmonics as TG
from tests import test_hip_gene_kinetics as TQ
from velocycle_amd import gene_harmonics as GH
from velocycle_amd import gene_kinetics as GK
from velocycle_amd.gene_batch import GeneBatchHarmonicFit
from velocycle_amd.phase_mle import phase_mle

pytestmark = pytest.mark.gpu

EVALUATE_R = 2.0                 # of D.EVALUATE_AT: the evaluate-only call of vc_gene_dispersion
CASES = {
    "glm": ["shape_65_7_3_Poisson", "shape_65_7_3_NegativeBinomial", "shape_257_5_1_Poisson", "shape_257_5_1_NegativeBinomial",
            "per_gene_dispersion", "prior_wide"],       # per_gene_dispersion: no prior (NULL prior pointers); prior_wide: with them
    "batch": ["seven_2_Poisson", "seven_2_NegativeBinomial", "silent_batch", "nu_prior"],
    "dispersion": ["shape_65_7_3", "shape_257_5_1", "evaluate"],
    "kinetics": ["shape_65_4_2_Poisson", "shape_257_5_1_NegativeBinomial", "score_257_5_3"],      # score_257_5_3: three rows of w_dev
    "mle": ["65_257_100_NegativeBinomial", "65_257_100_Poisson", "63_7_33_NegativeBinomial", "63_7_33_Poisson"],
}
STORAGES = ("u16", "f32")
ALL = [(k, c, s) for k in CASES for c in CASES[k] for s in STORAGES]
GENE_KERNELS = [(k, c, s) for (k, c, s) in ALL if k != "mle"]
LAYOUTS = [L.padded(1), L.padded(3), L.padded(61), L.window(5, 7), L.offset_inputs, L.side_stream]
BIG_CASES = {"glm": "shape_257_5_1_NegativeBinomial", "batch": "one_batch", "dispersion": "shape_257_5_1",
             "kinetics": "shape_257_5_1_NegativeBinomial", "mle": "257_3_33_NegativeBinomial"}


def ids(params):
    return ["-".join(p) for p in params]


@lru_cache(maxsize=None)
def mle_problem(case):
    Nc, Ng, bins, noise = case.split("_")
    S, T, n = TM.problem(int(Nc), int(Ng), int(bins), seed=int(Nc) + int(Ng))
    return S, T, n, noise


@lru_cache(maxsize=None)
def spec(kernel, case, storage):
    if kernel == "glm":
        return L.glm_spec(G.cases()[case], storage)
    if kernel == "batch":
        return L.batch_spec(BC.cases()[case], storage)
    if kernel == "dispersion":
        if case == "evaluate":
            return L.dispersion_spec(D.cases()[D.EVALUATE_CASE], storage, start=1.0 / EVALUATE_R, evaluate_only=True)
        return L.dispersion_spec(D.cases()[case], storage)
    if kernel == "kinetics":
        return L.kinetics_spec(Q.cases()[case], storage)
    S, T, n, noise = mle_problem(case)
    return L.mle_spec(S, T, n, noise, 0.3, storage)


@lru_cache(maxsize=None)
def compact(kernel, case, storage):
    out = L.direct_call(spec(kernel, case, storage), L.compact)
    assert out["guards_intact"] and out["outside_untouched"] and out["gene_stride"] == spec(kernel, case, storage)["M"].shape[1]
    return out


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def constants(s, with_r=True):
    """The workers' own lgamma constants of a spec's float32 block, on the device."""
    dev = torch.device("cuda", torch.cuda.current_device())
    r32 = s.get("r32") if with_r else None
    return GH._constants(s["blk32"].to(dev), r32.to(dev).double() if r32 is not None else None).cpu().numpy()


def unpacked(packed, K):
    """[Ng, K (K + 1) / 2] packed row by row -> [Ng, K, K] symmetric."""
    tri = np.tril_indices(K)
    full = np.zeros((packed.shape[0], K, K))
    full[:, tri[0], tri[1]] = packed
    full[:, tri[1], tri[0]] = packed
    return full


# ------------------------------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES["glm"])
def test_anchor_gene_glm(case, storage):
    s, out = spec("glm", case, storage), compact("glm", case, storage)
    null = L.direct_call(L.glm_spec(G.cases()[case], storage, null=True), L.compact)
    assert null["guards_intact"]
    const, cov = constants(s), unpacked(out["cov"], s["K"])
    fit = GH.GeneHarmonicFit(means=out["nu"].T.copy(), stds=np.sqrt(np.einsum("gii->ig", cov)), cov=cov, loglik=out["ll"] + const,
                             loglik_null=null["ll"] + const, decrement=out["dec"], iterations=out["it"], status=out["st"])
    TG.assert_within_bars(case, fit)
    worker = TG.fitted(case)
    for name in ("means", "cov", "decrement", "iterations", "status"):
        assert bits(getattr(fit, name), getattr(worker, name)), name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES["batch"])
def test_anchor_gene_glm_batch(case, storage):
    s, out = spec("batch", case, storage), compact("batch", case, storage)
    null = L.direct_call(L.batch_spec(BC.cases()[case], storage, null=True), L.compact)
    assert null["guards_intact"]
    const, cov = constants(s), unpacked(out["cov"], s["K"])
    fit = GeneBatchHarmonicFit(means=out["nu"].T.copy(), stds=np.sqrt(np.einsum("gii->ig", cov)), cov=cov, loglik=out["ll"] + const,
                               loglik_null=null["ll"] + const, decrement=out["dec"], iterations=out["it"], status=out["st"],
                               delta_nu=out["delta"].T.copy(), delta_nu_stds=np.sqrt(out["dvar"]).T.copy())
    TB.assert_within_bars(case, fit)
    worker = TB.fitted(case)
    for name in ("means", "cov", "decrement", "iterations", "status", "delta_nu"):
        assert bits(getattr(fit, name), getattr(worker, name)), name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES["dispersion"])
def test_anchor_gene_dispersion(case, storage):
    s, out = spec("dispersion", case, storage), compact("dispersion", case, storage)
    fit = GH.GeneDispersionFit(dispersion=1.0 / out["r"].astype(np.float64), log_r=out["rho"], log_r_std=GH._info_to_std(out["info"]),
                               loglik=out["ll"] + constants(s, with_r=False), score=out["score"], iterations=out["it"], status=out["st"])
    if case == "evaluate":
        bars, worst = D.bars(), dict(loglik=0.0, score=0.0)
        for g in range(out["ll"].shape[0]):
            ref, _ = D.evaluated()[(EVALUATE_R, g)]
            d = D.point_distances(out["ll"][g], out["score"][g], ref)
            worst = {key: max(worst[key], d[key]) for key in worst}
            assert out["st"][g] == D.EVALUATED and out["it"][g] == 0 and out["r"][g] == np.float32(EVALUATE_R)
        print(f"evaluate-only at r = {EVALUATE_R}: loglik {worst['loglik']:.3g} (bar {bars['loglik']:.3g}), score {worst['score']:.3g} "
              f"(bar {bars['score']:.3g})")
        assert worst["loglik"] <= bars["loglik"] and worst["score"] <= bars["score"]
        worker = TD.run(D.EVALUATE_CASE, start=1.0 / EVALUATE_R, evaluate_only=True)
    else:
        TD.assert_within_bars(case, fit)
        worker = TD.run(case)
    for name in ("dispersion", "log_r", "log_r_std", "score", "iterations", "status"):
        assert bits(getattr(fit, name), getattr(worker, name)), name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES["kinetics"])
def test_anchor_gene_kinetics(case, storage):
    s, out = spec("kinetics", case, storage), compact("kinetics", case, storage)
    dev = torch.device("cuda", torch.cuda.current_device())
    names = ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")
    shell = SimpleNamespace(Ng=out["ll"].shape[0], dev=dev, const=torch.from_numpy(constants(s)).to(dev))
    fit = GK._Problem.fit(shell, {n: torch.from_numpy(out[n]).to(dev) for n in names})        # the worker's own packaging of the outputs
    assert fit.score_w.shape[1] == s["NW"] == Q.cases()[case]["W"].shape[0]
    TQ.assert_within_bars(case, fit)
    worker = TQ.run(case)
    for name in ("log_gamma", "log_beta", "cov", "decrement", "iterations", "status", "n_clamped", "score_w", "info_w"):
        assert bits(getattr(fit, name), getattr(worker, name)), name


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("case", CASES["mle"])
def test_anchor_phase_mle(case, storage):
    out = compact("mle", case, storage)
    S, T, n, noise = mle_problem(case)
    best, prof = out["best_bin"], torch.from_numpy(out["logp_rel"]).double()
    logP, absP = MC.logp64(S, T, n, 1.0, noise, 0.3)
    j = MC.judge(logP, absP, best.astype(np.int64))
    assert j["regret_ratio"].max() <= F.regret_bar(), j["regret_ratio"].max()
    assert float(prof.max()) == 0.0 and bool((prof[torch.as_tensor(best.astype(np.int64)), torch.arange(prof.shape[1])] == 0).all())
    err = ((prof - MC.profile64(logP)).abs() / (MC.EPS32 * torch.as_tensor(j["A"]))).max().item()
    assert err <= F.profile_bar(), err
    wbest, wprof = phase_mle(S, T, n, noisemodel=noise, dispersion=0.3, return_profile=True, storage=storage)
    assert np.array_equal(wbest.cpu().numpy(), best) and bits(wprof.cpu().numpy(), out["logp_rel"])


# ------------------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("layout", LAYOUTS, ids=[lay.name for lay in LAYOUTS])
@pytest.mark.parametrize("kernel,case,storage", ALL, ids=ids(ALL))
def test_layout_equals_compact(kernel, case, storage, layout):
    s = spec(kernel, case, storage)
    got = L.direct_call(s, layout)
    assert got["guards_intact"] and got["outside_untouched"]
    assert got["gene_stride"] == s["M"].shape[1] + layout.pad + layout.left + layout.right
    L.assert_same_outputs(got, compact(kernel, case, storage))


@pytest.mark.parametrize("single", [False, True], ids=["inner", "single"])
@pytest.mark.parametrize("kernel,case,storage", GENE_KERNELS, ids=ids(GENE_KERNELS))
def test_gene_range_equals_the_rows_of_the_whole_call(kernel, case, storage, single):
    s = spec(kernel, case, storage)
    Ng = s["M"].shape[0]
    g0, g1 = (1, 2) if single else (1, Ng - 1)
    assert 1 <= g0 < g1 < Ng
    got = L.direct_call(s, L.gene_range(g0, g1))
    assert got["guards_intact"] and got["outside_untouched"]
    whole = compact(kernel, case, storage)
    L.assert_same_outputs(got, {k: (v if k in L.OUTPUT_FLAGS else v[g0:g1]) for k, v in whole.items()})


# ---------------------------------------------------------------------------------------------------------- the 32-bit row index
@pytest.fixture(scope="module")
def big():
    """One allocation for the row-index tests of a module (this one's five; tests/test_hip_cabi_layouts_six.py takes the fixture over
    for its six): 2^31 + 2 gene_stride + Nc + BIG_U_OFFSET uint16 elements, every byte 0xFF; freed when the module is done."""
    free, _ = torch.cuda.mem_get_info()
    if free < L.BIG_FREE_NEEDED:
        pytest.skip(f"the 32-bit row-index tests need {L.BIG_FREE_NEEDED} bytes free on the device ({2 * L.BIG_TOTAL} in one allocation); "
                    f"{free} are free")
    t = L.big_allocation(torch.device("cuda", torch.cuda.current_device()))
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", list(BIG_CASES))
def test_row_index_beyond_32_bits(kernel, big):
    """uint16, Ng = 3, Nc = 257, gene_stride = 2^30 + 1, counts_dev 2^31 elements into the allocation: 2 gene_stride does not fit a signed
    32-bit integer, and what a truncated index addresses is inside the allocation and poison (tests/test_cabi_layouts_cpu.py)."""
    case = BIG_CASES[kernel]
    if kernel == "mle":
        s = spec(kernel, case, "u16")
    else:
        whole = L.batch_spec(BC.cases()[case], "u16") if kernel == "batch" else spec(kernel, case, "u16")
        s = L.take_genes(whole, 0, L.BIG_NG)
    assert s["M"].shape == (L.BIG_NG, L.BIG_NC) and s["M"].dtype == np.uint16
    want = L.direct_call(s, L.compact)
    got = L.direct_call(s, L.big_stride, big=big)
    assert got["gene_stride"] == 2 ** 30 + 1 and got["guards_intact"] and want["guards_intact"]
    L.assert_same_outputs(got, want)
