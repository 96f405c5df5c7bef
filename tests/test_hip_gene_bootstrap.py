"""GPU: the weighted per-gene harmonic fit (vc_gene_glm_weighted), `gene_harmonics(cell_weights=)`, `gene_harmonics_bootstrap` and
`Cycle.from_phases_mle(bootstrap=)`, judged by tests/gene_boot_checker.py: the float64 fit of the expanded data, with bars that are 4 x the
float32 restatement's own distance from it (tests/test_gene_bootstrap_cpu.py asserts their cap and the share of separated pairs)."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_boot_checker as W
from tests import gene_glm_checker as G
from tests.test_gene_bootstrap_cpu import REFUSALS, boot_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.gene_bootstrap import gene_harmonics_bootstrap
from velocycle_amd.gene_harmonics import _stage, _unpack_tri, check_arguments, gene_harmonics

pytestmark = pytest.mark.gpu
DONE = (G.CONVERGED, G.ROUNDING)
NAMES = ("nu", "cov", "ll", "dec", "it", "st")
GUARD = 5
PATTERN = {torch.float64: -1234.5, torch.int32: -77}


def harmonics_kw(p):
    prior = p["prior"] if p["prior"] is not None else (None, None)
    return dict(harmonics=p["H"], a=p["a"], noisemodel=p["noisemodel"], dispersion=p["dispersion"] if p["dispersion"] is not None else 0.3,
                prior_means=prior[0], prior_stds=prior[1])


def run(p, **kw):
    return gene_harmonics(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], **harmonics_kw(p), **kw)


def boot(p, **kw):
    return gene_harmonics_bootstrap(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], **harmonics_kw(p), **kw)


def stage(p, storage="auto"):
    """The device inputs of a problem, staged as the workers stage them."""
    S = p["S"].astype(np.float32)
    kw = harmonics_kw(p)
    basis, logm, r, pm, pp = check_arguments(S, G.directions(p["phis"]), p["n"], kw["harmonics"], kw["a"], kw["noisemodel"], kw["dispersion"],
                                             kw["prior_means"], kw["prior_stds"])
    dev = torch.device("cuda")
    Nc, Ng = S.shape
    _, kblk, kind = _stage(S, 0, Ng, Nc, dev, storage)
    f32 = lambda t: t.to(torch.float32).to(dev).contiguous() if t is not None else None          # noqa: E731
    f64 = lambda t: t.to(dev).contiguous() if t is not None else None                          # noqa: E731
    return dict(kblk=kblk, kind=kind, B=f32(basis), logm=f32(logm), r=f32(r), pm=f64(pm), pp=f64(pp), Nc=Nc, Ng=Ng, K=basis.shape[0],
                noise=_lib.NOISE[p["noisemodel"]])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(n, dtype):
    return torch.full((n + 2 * GUARD,), PATTERN[dtype], dtype=dtype, device="cuda")


def _launch(st, weights, g0, g1, R, sizes, w_ptr=None, wstride=None, start=None, want_cov=True, tol=1e-10, max_iter=25):
    """One call of vc_gene_glm (weights None) or vc_gene_glm_weighted on genes [g0, g1): host arrays by name.  Every output lies between
    guard bands of a fixed pattern, which must be intact afterwards."""
    lib = _lib.load()
    n, K = g1 - g0, st["K"]
    sl = lambda t: t[g0:g1] if t is not None else None                                            # noqa: E731
    bufs = {k: _guarded(R * n * sizes[k][0], sizes[k][1]) for k in NAMES}
    outs = [C.c_void_p(bufs[k].data_ptr() + GUARD * bufs[k].element_size()) if (want_cov or k != "cov") else None for k in NAMES]
    head = [_ptr(st["kblk"][g0:g1]), st["kind"], n, st["Nc"], st["Nc"], _ptr(st["B"]), K, _ptr(st["logm"]), st["noise"], _ptr(sl(st["r"])),
            _ptr(sl(st["pm"])), _ptr(sl(st["pp"]))]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if weights is None and w_ptr is None:
        rc = lib.vc_gene_glm(*head, float(tol), int(max_iter), *outs, stream)
    else:
        if w_ptr is None:
            w_d = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).cuda()
            w_ptr, wstride = _ptr(w_d), st["Nc"]
        s_d = torch.from_numpy(np.ascontiguousarray(start[g0:g1], dtype=np.float64)).cuda() if start is not None else None
        rc = lib.vc_gene_glm_weighted(*head, w_ptr, R, wstride, _ptr(s_d), float(tol), int(max_iter), *outs, stream)
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    got = {}
    for k in NAMES:
        host = bufs[k].cpu().numpy()
        assert (host[:GUARD] == PATTERN[sizes[k][1]]).all() and (host[-GUARD:] == PATTERN[sizes[k][1]]).all(), f"guard band of {k}"
        body = host[GUARD:-GUARD]
        if k == "cov" and not want_cov:
            assert (body == PATTERN[torch.float64]).all(), "cov_dev NULL: nothing may be stored"
        got[k] = body.reshape(R, n, sizes[k][0]) if sizes[k][0] > 1 else body.reshape(R, n)
    return got


def weighted(st, weights, g0=0, g1=None, **kw):
    g1 = st["Ng"] if g1 is None else g1
    K = st["K"]
    sizes = dict(nu=(K, torch.float64), cov=(K * (K + 1) // 2, torch.float64), ll=(1, torch.float64), dec=(1, torch.float64),
                 it=(1, torch.int32), st=(1, torch.int32))
    R = kw.pop("R", None) or np.asarray(weights).shape[0]
    out = _launch(st, weights, g0, g1, R, sizes, **kw)
    if K == 1:
        out["nu"], out["cov"] = out["nu"].reshape(R, g1 - g0, 1), out["cov"].reshape(R, g1 - g0, 1)
    return out


def plain(st):
    out = weighted(st, None, R=1)
    return out


def same(a, b, what=""):
    for k in NAMES:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def same_fit(a, b):
    for f in fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f.name


def stds_of(cov_packed, K):
    full = _unpack_tri(torch.from_numpy(np.ascontiguousarray(cov_packed)), K).numpy()
    return np.sqrt(np.einsum("gii->gi", full))


@lru_cache(maxsize=None)
def unweighted_means(name):
    """[Ng, K]: the warm start of a case, the unweighted fit of its problem."""
    return np.ascontiguousarray(run(W.cases()[name][0]).means.T)


def check_left_out(got, b, g):
    """A pair whose float64 reference did not converge: a documented status and the outputs the contract gives it."""
    st = got["st"][b, g]
    assert st in (G.CONVERGED, G.ROUNDING, G.UNBOUNDED, G.SINGULAR, G.MAX_ITER), st
    if st == G.UNBOUNDED and np.isnan(got["ll"][b, g]):                        # no weighted count at all: the outputs of an empty gene
        assert got["it"][b, g] == 0 and np.isnan(got["cov"][b, g]).all() and np.isnan(got["dec"][b, g]) and (got["nu"][b, g, 1:] == 0).all()
        return
    assert np.isfinite(got["nu"][b, g]).all() and got["it"][b, g] >= 0          # otherwise a point was reached
    assert np.isnan(got["cov"][b, g]).all() if st == G.SINGULAR else np.isfinite(got["cov"][b, g]).all()
    assert np.isfinite(got["ll"][b, g])


@pytest.mark.parametrize("name", list(W.cases()))
def test_bars(name):
    p, Wt = W.cases()[name]
    solved, keep, bars = W.solved(name), W.bearing(name), W.bars()
    R, Ng, K = Wt.shape[0], p["S"].shape[1], 2 * p["H"] + 1
    fits = [run(p, cell_weights=w) for w in Wt]
    worst = dict(coef=0.0, std=0.0, loglik=0.0, lr=0.0)
    for b, fit in enumerate(fits):                                  # the worker: loglik and lr_stat with the weighted constants
        for g in range(Ng):
            if not keep[b, g]:
                continue
            f64, n64 = solved[b][g][:2]
            assert fit.status[g] in DONE and fit.iterations[g] <= W.iteration_bound(name, b, g), (name, b, g, fit.status[g], fit.iterations[g])
            d = G.distances(fit.means[:, g], fit.stds[:, g], fit.loglik[g], fit.lr_stat[g], f64, n64)
            worst = {key: max(worst[key], d[key]) for key in worst}
    storages = ("u16", "f32") if p["S"].max() <= 65535 else ("f32",)
    first = None
    for storage in storages:
        st = stage(p, storage)
        for start in (None, unweighted_means(name)):
            got = weighted(st, Wt, start=start)
            if start is None:
                first = first or got
                same(first, got, storage)                           # the other storage: the same bits
                for b, fit in enumerate(fits):                      # and the worker's one-row calls are rows of this call
                    assert np.ascontiguousarray(got["nu"][b].T).tobytes() == fit.means.tobytes() and np.array_equal(got["st"][b], fit.status)
            for b in range(R):
                sd = stds_of(got["cov"][b], K)
                for g in range(Ng):
                    if not keep[b, g]:
                        check_left_out(got, b, g)
                        continue
                    f64, n64 = solved[b][g][:2]
                    assert got["st"][b, g] in DONE, (name, storage, start is not None, b, g, got["st"][b, g])
                    assert got["it"][b, g] <= W.iteration_bound(name, b, g, warm=start is not None), (name, b, g, got["it"][b, g])
                    const = fits[b].loglik[g] - first["ll"][b, g]   # the weighted constants the kernel leaves out
                    d = G.distances(got["nu"][b, g], sd[g], got["ll"][b, g] + const, fits[b].lr_stat[g], f64, n64)
                    worst = {key: max(worst[key], d[key]) for key in worst}
    print(f"{name}: worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    for key in worst:
        assert worst[key] <= bars[key], (name, key, worst[key], bars[key])


@pytest.mark.parametrize("noise,disp", G.NOISES)
@pytest.mark.parametrize("Nc,Ng,H", G.SHAPES)
def test_unit_weights_are_the_unweighted_fit(Nc, Ng, H, noise, disp):
    p = G.cases()[f"shape_{Nc}_{Ng}_{H}_{noise}"]
    for storage in ("u16", "f32"):
        st = stage(p, storage)
        same(plain(st), weighted(st, np.ones((1, Nc))), storage)
    same_fit(run(p), run(p, cell_weights=np.ones(Nc)))


@pytest.mark.parametrize("name", ["shape_65_7_3_NegativeBinomial", "shape_257_5_1_Poisson"])
def test_rows_and_cuts(name):
    p, Wt = W.cases()[name]
    Nc, Ng = p["S"].shape
    st = stage(p, "u16")
    whole = weighted(st, Wt)
    same(whole, weighted(st, Wt), "repetition")
    same(whole, weighted(stage(p, "f32"), Wt), "storage")
    rows = [weighted(st, Wt[b:b + 1]) for b in range(Wt.shape[0])]
    same(whole, {k: np.concatenate([r[k] for r in rows], axis=0) for k in NAMES}, "rows")
    genes = [weighted(st, Wt, g, g + 1) for g in range(Ng)]          # a separated pair leaves its neighbours' bits alone
    same(whole, {k: np.concatenate([x[k] for x in genes], axis=1) for k in NAMES}, "genes")
    warm = unweighted_means("shape_65_7_3_NegativeBinomial" if Ng == 7 else "shape_257_5_1_Poisson")
    whole_w = weighted(st, Wt, start=warm)
    same(whole_w, {k: np.concatenate([weighted(st, Wt, g, g + 1, start=warm)[k] for g in range(Ng)], axis=1) for k in NAMES}, "warm genes")
    without = weighted(st, Wt, want_cov=False)                      # cov_dev NULL changes nothing else
    for k in NAMES:
        assert k == "cov" or without[k].tobytes() == whole[k].tobytes(), k
    # a stride of Nc + 3 with NaN padding, the table advanced inside a larger one
    R = Wt.shape[0]
    big = np.full((R + 2, Nc + 3), np.nan, dtype=np.float32)
    big[1:R + 1, :Nc] = Wt
    big_d = torch.from_numpy(big).cuda()
    same(whole, weighted(st, None, R=R, w_ptr=C.c_void_p(big_d.data_ptr() + 4 * (Nc + 3)), wstride=Nc + 3), "stride")


def test_more_genes_than_one_launch_holds():
    """The entry point launches slabs of 65535 genes (the second grid dimension): a call over 65541 genes equals its cuts at the slab
    boundary and elsewhere bit for bit, every pair is solved, and the worker's default chunk goes through the same call."""
    Nc, Ng = 3, 65535 + 6
    rng = np.random.default_rng(5)
    p = G.problem(rng.poisson(2.0, (Nc, Ng)) + 1.0, np.array([0.1, 2.0, 4.0]), np.array([1.0, 2.0, 3.0]), 0, "Poisson")
    Wt = np.array([[1.0, 0.0, 2.0], [1.0, 1.0, 1.0], [0.5, 3.0, 0.0]])
    st = stage(p)
    whole = weighted(st, Wt)
    assert set(np.unique(whole["st"])) <= set(DONE) and np.isfinite(whole["nu"]).all() and np.isfinite(whole["cov"]).all()
    for cut in (65535, 40000):
        parts = [weighted(st, Wt, 0, cut), weighted(st, Wt, cut, Ng)]
        same(whole, {k: np.concatenate([x[k] for x in parts], axis=1) for k in NAMES}, cut)
    one = plain(st)
    for k in NAMES:
        assert whole[k][1].tobytes() == one[k][0].tobytes(), k        # the row of ones is vc_gene_glm's answer, beyond the first slab too
    bs = boot(p, weights=Wt, fit=type("F", (), {"means": np.full((1, Ng), np.nan)})())          # no usable start: the default start
    assert bs.replicates.tobytes() == np.ascontiguousarray(whole["nu"].transpose(0, 2, 1)).tobytes() and np.array_equal(bs.status, whole["st"])


def test_planted_rows():
    S, phis, n = G.separated()
    p = G.problem(S, phis, n, 1, "Poisson")
    Nc, Ng = S.shape
    Wt = np.ones((3, Nc))
    Wt[1, [10, 100, 200]] = 0.0                                     # the sixth gene's only counts
    Wt[2] = 0.0
    st = stage(p)
    got = weighted(st, Wt)

    def is_empty(b, g):
        return (got["st"][b, g] == G.UNBOUNDED and got["it"][b, g] == 0 and np.isnan(got["cov"][b, g]).all() and np.isnan(got["ll"][b, g])
                and np.isnan(got["dec"][b, g]) and not np.isfinite(got["nu"][b, g, 0]) and (got["nu"][b, g, 1:] == 0).all())

    assert is_empty(1, Ng - 1) and all(is_empty(2, g) for g in range(Ng))
    for k in NAMES:                                                 # the five other genes of row 1 lose three cells and nothing else
        assert np.isfinite(got[k][1, :Ng - 1]).all(), k
    assert set(got["st"][1, :Ng - 1]) <= set(DONE) and set(got["st"][0, :Ng - 1]) <= set(DONE)
    one = plain(st)
    for k in NAMES:
        assert got[k][0].tobytes() == one[k][0].tobytes(), k
    # a non-finite start, or one outside the bound, falls back to the default start's bits
    start = np.ascontiguousarray(run(p).means.T)
    bad = start.copy()
    bad[0, 1], bad[1, 0], bad[2, 2], bad[3, 1] = np.nan, np.inf, 50.5, -np.inf
    warm, mixed = weighted(st, Wt[:2], start=start), weighted(st, Wt[:2], start=bad)
    for k in NAMES:
        assert mixed[k][:, :4].tobytes() == got[k][:2, :4].tobytes() and mixed[k][:, 4:].tobytes() == warm[k][:, 4:].tobytes(), k
    # one cell, no harmonics: weight 0 has no maximum, weight 2 the maximum of weight 1
    p1 = G.problem(np.array([[3.0]]), np.array([0.3]), np.array([1.0]), 0, "Poisson")
    g1 = weighted(stage(p1), np.array([[0.0], [2.0], [1.0]]))
    assert g1["st"][0, 0] == G.UNBOUNDED and np.isnan(g1["ll"][0, 0]) and np.isnan(g1["cov"][0, 0]).all()
    assert g1["st"][1, 0] in DONE and g1["st"][2, 0] in DONE
    assert abs(g1["nu"][1, 0, 0] - np.log(3.0)) <= 1e-12 and abs(g1["nu"][2, 0, 0] - np.log(3.0)) <= 1e-12      # logm = 0: nu_0 = ln 3
    assert abs(g1["cov"][1, 0, 0] * 6.0 - 1.0) <= 1e-6 and abs(g1["cov"][2, 0, 0] * 3.0 - 1.0) <= 1e-6       # 1 / (w mu), mu float32


def test_drawn_weights():
    name = "shape_257_5_1_NegativeBinomial"
    p = G.cases()[name]
    fit = run(p)
    b8 = boot(p, n_boot=8, seed=3, fit=fit, return_weights=True)
    again = boot(p, n_boot=8, seed=3, fit=fit, return_weights=True)
    assert b8.fit is fit and b8.replicates.shape == (8, 3, 5) and b8.status.shape == b8.iterations.shape == (8, 5)
    for f in ("replicates", "status", "iterations", "weights"):
        assert getattr(b8, f).tobytes() == getattr(again, f).tobytes(), f
    b4 = boot(p, n_boot=4, seed=3, fit=fit, return_weights=True, chunk_genes=2, storage="f32")
    for f in ("replicates", "status", "iterations", "weights"):
        assert getattr(b8, f)[:4].tobytes() == getattr(b4, f).tobytes(), f
    other = boot(p, n_boot=8, seed=4, fit=fit, return_weights=True)
    assert not np.array_equal(other.weights, b8.weights) and not np.array_equal(other.replicates, b8.replicates)
    w = b8.weights
    assert w.dtype == np.float32 and w.shape == (8, 257) and (w >= 0).all() and np.array_equal(w, np.round(w)) and 0.8 < w.mean() < 1.2
    assert boot(p, n_boot=2, seed=3, fit=fit).weights is None
    # the worker is one call of the entry point on that table, warm-started from the fit
    direct = weighted(stage(p), w, start=np.ascontiguousarray(fit.means.T))
    assert np.array_equal(direct["nu"].transpose(0, 2, 1), b8.replicates) and np.array_equal(direct["st"], b8.status)
    assert np.array_equal(direct["it"], b8.iterations)
    assert np.array_equal(boot(p, weights=w, fit=fit).replicates, b8.replicates)          # and the same table handed over
    # within the bars of the float64 reference on the read-back weights
    bars, worst = W.bars(), 0.0
    for b in range(8):
        for g in range(5):
            k, B, logm, r, prior = G._gene_inputs(p, g)
            f64 = G.newton64(*W.expand(k, B, logm, w[b]), p["noisemodel"], r, prior)
            assert f64["status"] == G.CONVERGED and b8.status[b, g] in DONE
            d = b8.replicates[b, :, g] - f64["nu"]
            worst = max(worst, float(np.sqrt(max(d @ f64["hess"] @ d, 0.0))))
    print(f"drawn weights: worst coef {worst:.3g} (bar {bars['coef']:.3g})")
    assert worst <= bars["coef"]
    assert (b8.n_ok == 8).all() and np.isfinite(b8.stds).all() and (b8.stds > 0).all()
    # fit=None runs the unweighted fit first
    auto = boot(p, n_boot=2, seed=3)
    same_fit(auto.fit, fit)
    assert auto.replicates.tobytes() == b8.replicates[:2].tobytes()


def test_containers():
    p = G.cases()["shape_257_5_1_NegativeBinomial"]
    S = p["S"].astype(np.float32)
    obs = pd.DataFrame({"n_scounts": p["n"]}, index=[f"c{i}" for i in range(S.shape[0])])
    ph = Phases.from_array(G.directions(p["phis"]), cell_names=list(obs.index))
    got = {}
    for kind, layer in (("dense", S), ("csr", sp.csr_matrix(S))):
        ad = AnnDataLite(layer, layer, obs=obs.copy())
        got[kind] = Cycle.from_phases_mle(ph, ad, 1, 1, "NegativeBinomial", 0.3, return_fit=True, bootstrap=16, bootstrap_seed=5)
        got[kind + "_plain"] = Cycle.from_phases_mle(ph, ad, 1, 1, "NegativeBinomial", 0.3, return_fit=True)
    (cyc, fit), (cyc0, fit0) = got["dense"], got["dense_plain"]
    assert fit0.bootstrap is None and "bootstrap" not in [f.name for f in fields(fit)]
    same_fit(fit, fit0)
    assert cyc.means.equals(cyc0.means) and not cyc.stds.equals(cyc0.stds)
    bs = fit.bootstrap
    assert bs.replicates.shape == (16, 3, 5) and bs.fit is fit
    assert np.array_equal(cyc.stds.values, Cycle.from_array(fit.means, bs.stds, gene_names=cyc.means.columns).stds.values)
    assert np.array_equal(cyc0.stds.values, Cycle.from_array(fit.means, fit.stds, gene_names=cyc.means.columns).stds.values)
    ref = boot(p, n_boot=16, seed=5, fit=fit0)
    assert ref.replicates.tobytes() == bs.replicates.tobytes()
    (cyc2, fit2) = got["csr"]
    assert fit2.bootstrap.replicates.tobytes() == bs.replicates.tobytes() and cyc2.stds.equals(cyc.stds) and cyc2.means.equals(cyc.means)
    with pytest.raises(ValueError, match="mle"):
        Cycle.from_phases_mle(ph, ad, 1, 1, "NegativeBinomial", "mle", bootstrap=4)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    assert lib.vc_gene_glm_weighted(*boot_args(noise=_lib.NOISE["Lognormal"])) == _lib.VC_ERR_UNSUPPORTED and b"Lognormal" in lib.vc_last_error(None)
    for kw, msg in REFUSALS:
        assert lib.vc_gene_glm_weighted(*boot_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
