"""GPU: the weighted batch-aware per-gene harmonic fit (vc_gene_glm_batch_weighted), `gene_harmonics_batched(cell_weights=)`,
`gene_harmonics_batched_bootstrap` and `Cycle.from_phases_batch_mle(bootstrap=)`, judged by tests/gene_batch_boot_checker.py: the float64
fit of the expanded data over the K + Nb coefficients, with bars that are 4 x the float32 restatement's own distance from it
(tests/test_gene_batch_bootstrap_cpu.py asserts their cap and that no pair is left out)."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from tests import gene_batch_boot_checker as Q
from tests import gene_batch_checker as BC
from tests import gene_glm_checker as G
from tests.test_gene_batch_bootstrap_cpu import REFUSALS, batch_boot_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import Cycle, Phases
from velocycle_amd.gene_batch import batch_labels, batch_segments, delta_prior, gene_harmonics_batched
from velocycle_amd.gene_bootstrap import draw_weights, gene_harmonics_batched_bootstrap
from velocycle_amd.gene_harmonics import _stage, _unpack_tri, check_arguments

pytestmark = pytest.mark.gpu
DONE = (G.CONVERGED, G.ROUNDING)
NAMES = ("nu", "delta", "cov", "dvar", "ll", "dec", "it", "st")
GUARD = 5
PATTERN = {torch.float64: -1234.5, torch.int32: -77}
BOOT_FIELDS = ("replicates", "delta_replicates", "status", "iterations")


def batched_kw(p):
    prior = p["prior"] if p["prior"] is not None else (None, None)
    return dict(harmonics=p["H"], a=p["a"], noisemodel=p["noisemodel"], dispersion=p["dispersion"] if p["dispersion"] is not None else 0.3,
                delta_nu_prior=p["dprior"], prior_means=prior[0], prior_stds=prior[1])


def run(p, **kw):
    return gene_harmonics_batched(p["S"].astype(np.float32), G.directions(p["phis"]), p["n"], p["labels"], **batched_kw(p), **kw)


def boot(p, counts=None, **kw):
    return gene_harmonics_batched_bootstrap(p["S"].astype(np.float32) if counts is None else counts, G.directions(p["phis"]), p["n"],
                                            p["labels"], **batched_kw(p), **kw)


def stage(p, storage="auto"):
    """The device inputs of a problem, staged and sorted by batch as the workers stage them; `perm` maps sorted cells to the caller's."""
    S = p["S"].astype(np.float32)
    kw = batched_kw(p)
    basis, logm, r, pm, pp = check_arguments(S, G.directions(p["phis"]), p["n"], kw["harmonics"], kw["a"], kw["noisemodel"], kw["dispersion"],
                                             kw["prior_means"], kw["prior_stds"])
    dev = torch.device("cuda")
    Nc, Ng = S.shape
    labels, Nb = batch_labels(p["labels"], Nc)
    dm, dq = delta_prior(p["dprior"], Nb, Ng)
    perm, seg = batch_segments(labels, Nb)
    _, kblk, kind = _stage(S, 0, Ng, Nc, dev, storage)
    kblk = kblk[:, torch.from_numpy(perm).to(dev)].contiguous()
    f32 = lambda t: t.to(torch.float32).to(dev).contiguous() if t is not None else None          # noqa: E731
    f64 = lambda t: t.to(dev).contiguous() if t is not None else None                          # noqa: E731
    return dict(kblk=kblk, kind=kind, B=f32(basis[:, perm]), logm=f32(logm[perm]), r=f32(r), pm=f64(pm), pp=f64(pp), dm=f64(dm), dq=f64(dq),
                Nc=Nc, Ng=Ng, Nb=Nb, K=basis.shape[0], perm=perm, seg=seg, noise=_lib.NOISE[p["noisemodel"]])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(n, dtype):
    return torch.full((n + 2 * GUARD,), PATTERN[dtype], dtype=dtype, device="cuda")


def launch(st, weights, g0=0, g1=None, start=None, want_var=True, R=None, w_ptr=None, wstride=None, counts=None, gene_stride=None,
           stream=None, tol=1e-10, max_iter=25):
    """One call of vc_gene_glm_batch (weights and w_ptr None) or vc_gene_glm_batch_weighted on genes [g0, g1): host arrays by name, of
    the shape [R, n, ...].  weights: [R, Nc] in the CALLER's cell order (sorted here).  start: (nu [Ng, K], delta [Ng, Nb]).  Every
    output lies between guard bands of a fixed pattern, which must be intact afterwards."""
    lib = _lib.load()
    g1 = st["Ng"] if g1 is None else g1
    n, K, Nb, Nc = g1 - g0, st["K"], st["Nb"], st["Nc"]
    is_plain = weights is None and w_ptr is None
    R = 1 if is_plain else (R or np.asarray(weights).shape[0])
    sizes = dict(nu=(K, torch.float64), delta=(Nb, torch.float64), cov=(K * (K + 1) // 2, torch.float64), dvar=(Nb, torch.float64),
                 ll=(1, torch.float64), dec=(1, torch.float64), it=(1, torch.int32), st=(1, torch.int32))
    sl = lambda t: t[g0:g1] if t is not None else None                                            # noqa: E731
    bufs = {k: _guarded(R * n * sizes[k][0], sizes[k][1]) for k in NAMES}
    outs = [C.c_void_p(bufs[k].data_ptr() + GUARD * bufs[k].element_size()) if (want_var or k not in ("cov", "dvar")) else None for k in NAMES]
    seg = (C.c_int64 * (Nb + 1))(*st["seg"])
    cnt = _ptr(st["kblk"][g0:g1]) if counts is None else counts
    head = [cnt, st["kind"], n, Nc, Nc if gene_stride is None else gene_stride, _ptr(st["B"]), K, _ptr(st["logm"]), st["noise"],
            _ptr(sl(st["r"])), Nb, seg, _ptr(st["dm"][g0:g1]), _ptr(st["dq"][g0:g1]), _ptr(sl(st["pm"])), _ptr(sl(st["pp"]))]
    s = torch.cuda.current_stream() if stream is None else stream
    sp_ = C.c_void_p(s.cuda_stream)
    if is_plain:
        rc = lib.vc_gene_glm_batch(*head, float(tol), int(max_iter), *outs, sp_)
    else:
        if w_ptr is None:
            w_d = torch.from_numpy(np.ascontiguousarray(np.asarray(weights)[:, st["perm"]], dtype=np.float32)).cuda()
            w_ptr, wstride = _ptr(w_d), Nc
        sn = torch.from_numpy(np.ascontiguousarray(start[0][g0:g1], dtype=np.float64)).cuda() if start is not None else None
        sd = torch.from_numpy(np.ascontiguousarray(start[1][g0:g1], dtype=np.float64)).cuda() if start is not None else None
        torch.cuda.synchronize()
        rc = lib.vc_gene_glm_batch_weighted(*head, w_ptr, R, wstride, _ptr(sn), _ptr(sd), float(tol), int(max_iter), *outs, sp_)
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    got = {}
    for k in NAMES:
        host = bufs[k].cpu().numpy()
        assert (host[:GUARD] == PATTERN[sizes[k][1]]).all() and (host[-GUARD:] == PATTERN[sizes[k][1]]).all(), f"guard band of {k}"
        body = host[GUARD:-GUARD]
        if k in ("cov", "dvar") and not want_var:
            assert (body == PATTERN[torch.float64]).all(), "NULL variance outputs: nothing may be stored"
        got[k] = body.reshape(R, n, sizes[k][0]) if k in ("nu", "delta", "cov", "dvar") else body.reshape(R, n)
    return got


def same(a, b, what="", names=NAMES):
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def same_fit(a, b):
    for f in fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f.name


def same_boot(a, b, rows=slice(None)):
    for f in BOOT_FIELDS:
        assert getattr(a, f)[rows].tobytes() == getattr(b, f).tobytes(), f


def stds_of(cov_packed, K):
    full = _unpack_tri(torch.from_numpy(np.ascontiguousarray(cov_packed)), K).numpy()
    return np.sqrt(np.einsum("gii->gi", full))


@lru_cache(maxsize=None)
def unweighted(name):
    """(nu [Ng, K], delta [Ng, Nb]): the warm start of a case, the device's unweighted fit of its problem."""
    fit = run(Q.cases()[name][0])
    return np.ascontiguousarray(fit.means.T), np.ascontiguousarray(fit.delta_nu.T)


@pytest.mark.parametrize("name", list(Q.cases()))
def test_bars(name):
    """Every (row, gene) pair of the case within the bars of the float64 fit of the expanded data: the worker's one-row calls (default
    start, the weighted constants and the weighted null model) and the entry point's R-row calls from the default and the warm start,
    in both storages where the counts allow uint16.  No pair is left out."""
    p, Wt = Q.cases()[name]
    solved, keep, bars = Q.solved(name), Q.bearing(name), Q.bars()
    assert keep.all()
    R, Ng, K = Wt.shape[0], p["S"].shape[1], 2 * p["H"] + 1
    fits = [run(p, cell_weights=w) for w in Wt]
    worst = dict.fromkeys(Q.YARDSTICKS, 0.0)
    for b, fit in enumerate(fits):
        for g in range(Ng):
            f64, n64 = solved[b][g][:2]
            assert fit.status[g] in DONE and fit.iterations[g] <= Q.iteration_bound(name, b, g), (name, b, g, fit.status[g], fit.iterations[g])
            d = BC.distances(fit.means[:, g], fit.delta_nu[:, g], fit.stds[:, g], fit.delta_nu_stds[:, g], fit.loglik[g], fit.lr_stat[g], f64, n64)
            worst = {key: max(worst[key], d[key]) for key in worst}
    for b, lost in enumerate(Q.emptied(name)):                       # an emptied batch: its offset at the prior mean, its variance the prior's
        for bb in np.flatnonzero(lost):
            m, s = (np.broadcast_to(np.asarray(v, dtype=np.float64), (len(lost), Ng))[bb] for v in p["dprior"])
            assert np.allclose(fits[b].delta_nu[bb], m, rtol=0, atol=1e-6) and np.all(fits[b].delta_nu_stds[bb] >= 0.999999 * s)
    storages = ("u16", "f32") if p["S"].max() <= 65535 else ("f32",)
    first = None
    for storage in storages:
        st = stage(p, storage)
        for start in (None, unweighted(name)):
            got = launch(st, Wt, start=start)
            if start is None:
                first = first or got
                same(first, got, storage)                           # the other storage: the same bits
                for b, fit in enumerate(fits):                      # and the worker's one-row calls are rows of this call
                    assert np.ascontiguousarray(got["nu"][b].T).tobytes() == fit.means.tobytes() and np.array_equal(got["st"][b], fit.status)
                    assert np.ascontiguousarray(got["delta"][b].T).tobytes() == fit.delta_nu.tobytes()
            for b in range(R):
                sd = stds_of(got["cov"][b], K)
                for g in range(Ng):
                    f64, n64 = solved[b][g][:2]
                    assert got["st"][b, g] in DONE, (name, storage, start is not None, b, g, got["st"][b, g])
                    assert got["it"][b, g] <= Q.iteration_bound(name, b, g, warm=start is not None), (name, b, g, got["it"][b, g])
                    const = fits[b].loglik[g] - first["ll"][b, g]   # the weighted constants the kernel leaves out
                    ll = got["ll"][b, g] + const
                    d = BC.distances(got["nu"][b, g], got["delta"][b, g], sd[g], np.sqrt(got["dvar"][b, g]), ll,
                                     2 * (ll - fits[b].loglik_null[g]), f64, n64)
                    worst = {key: max(worst[key], d[key]) for key in worst}
    print(f"{name}: worst " + ", ".join(f"{k} {v:.3g} (bar {bars[k]:.3g})" for k, v in worst.items()))
    for key in worst:
        assert worst[key] <= bars[key], (name, key, worst[key], bars[key])


@pytest.mark.parametrize("noise,disp", BC.NOISES)
@pytest.mark.parametrize("H", [0, 1, 2, 3])
def test_unit_weights_are_the_unweighted_fit(H, noise, disp):
    """A table of ones, R = 1, no start: all eight outputs are vc_gene_glm_batch's bit for bit, on the 961 cells in batches of
    1, 63, 64, 65, 255, 256, 257, in both storages."""
    sim = BC.simulated(BC.SEVEN, 5)
    p = BC.problem(sim["S"], sim["phis"], sim["n"], sim["labels"], H, noise, disp)
    for storage in ("u16", "f32"):
        st = stage(p, storage)
        plain = launch(st, None)
        assert set(plain["st"].reshape(-1)) <= set(DONE)
        same(plain, launch(st, np.ones((1, 961))), storage)


def test_rows_and_cuts():
    name = "seven_1_NegativeBinomial"
    p, Wt = Q.cases()[name]
    Ng = p["S"].shape[1]
    st = stage(p, "u16")
    whole = launch(st, Wt)
    same(whole, launch(st, Wt), "repetition")
    same(whole, launch(stage(p, "f32"), Wt), "storage")
    rows = [launch(st, Wt[b:b + 1]) for b in range(Wt.shape[0])]
    same(whole, {k: np.concatenate([r[k] for r in rows], axis=0) for k in NAMES}, "rows")
    cut = [launch(st, Wt, 0, 2), launch(st, Wt, 2, Ng)]
    same(whole, {k: np.concatenate([x[k] for x in cut], axis=1) for k in NAMES}, "genes 2 + 3")
    warm = unweighted(name)
    whole_w = launch(st, Wt, start=warm)
    assert whole_w["it"].sum() < whole["it"].sum()                  # the warm start is used
    same(whole_w, launch(st, Wt, start=warm), "warm repetition")
    cut = [launch(st, Wt, 0, 2, start=warm), launch(st, Wt, 2, Ng, start=warm)]
    same(whole_w, {k: np.concatenate([x[k] for x in cut], axis=1) for k in NAMES}, "warm genes 2 + 3")
    rows = [launch(st, Wt[b:b + 1], start=warm) for b in range(Wt.shape[0])]
    same(whole_w, {k: np.concatenate([r[k] for r in rows], axis=0) for k in NAMES}, "warm rows")
    without = launch(st, Wt, want_var=False)                        # NULL variance outputs change nothing else
    same(whole, without, "no variances", [k for k in NAMES if k not in ("cov", "dvar")])
    # a start that is not usable (a NaN harmonic, an offset beyond the bound) is the default start, gene by gene
    bad = (warm[0].copy(), warm[1].copy())
    bad[0][0, 1], bad[1][1, 6], bad[1][2, 0] = np.nan, 50.5, -np.inf
    mixed = launch(st, Wt, start=bad)
    for k in NAMES:
        assert mixed[k][:, :3].tobytes() == whole[k][:, :3].tobytes() and mixed[k][:, 3:].tobytes() == whole_w[k][:, 3:].tobytes(), k


@pytest.mark.parametrize("storage", ["u16", "f32"])
def test_padded_layout_on_another_stream(storage):
    """gene_stride = Nc + 37 with the padding poisoned, weight_stride = Nc + 5 with NaN in the padding, a non-default stream: the bits of
    the dense layout, and nothing written outside [R][Ng]... (the guard bands of `launch`)."""
    name = "seven_1_NegativeBinomial"
    p, Wt = Q.cases()[name]
    st = stage(p, storage)
    Nc, Ng, R = st["Nc"], st["Ng"], Wt.shape[0]
    dense = launch(st, Wt, start=unweighted(name))
    if storage == "u16":
        wide = torch.full((Ng, Nc + 37), -1, dtype=torch.int16, device="cuda")                    # 65535 in every padding element
        wide[:, :Nc] = st["kblk"].view(torch.int16)
    else:
        wide = torch.full((Ng, Nc + 37), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, :Nc] = st["kblk"]
    big = np.full((R, Nc + 5), np.nan, dtype=np.float32)
    big[:, :Nc] = Wt[:, st["perm"]]
    big_d = torch.from_numpy(big).cuda()
    other = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = launch(st, None, R=R, w_ptr=_ptr(big_d), wstride=Nc + 5, counts=_ptr(wide), gene_stride=Nc + 37, stream=other, start=unweighted(name))
    same(dense, got, storage)


def test_planted_rows():
    """A NaN-weight row and an all-zero row among good rows: the documented UNBOUNDED outputs, whatever the start holds, and the
    neighbours' bits unchanged."""
    name = "interleaved"
    p, Wt = Q.cases()[name]
    Nc, Ng = p["S"].shape
    st = stage(p)
    planted = np.vstack([Wt[0], np.zeros(Nc), Wt[1], Wt[2]])
    planted[3, 17] = np.nan
    m = np.broadcast_to(np.asarray(p["dprior"][0], dtype=np.float64), (st["Nb"],))
    for start in (None, unweighted(name)):
        got = launch(st, planted, start=start)
        good = launch(st, Wt[:2], start=start)
        for k in NAMES:
            assert got[k][0].tobytes() == good[k][0].tobytes() and got[k][2].tobytes() == good[k][1].tobytes(), k
        for b in (1, 3):
            assert (got["st"][b] == G.UNBOUNDED).all() and (got["it"][b] == 0).all()
            assert np.isnan(got["cov"][b]).all() and np.isnan(got["dvar"][b]).all() and np.isnan(got["ll"][b]).all() and np.isnan(got["dec"][b]).all()
            assert not np.isfinite(got["nu"][b, :, 0]).any() and (got["nu"][b, :, 1:] == 0).all()
            assert (got["delta"][b] == m[None, :]).all()
        assert set(got["st"][[0, 2]].reshape(-1)) <= set(DONE)


def test_more_genes_than_one_launch_holds():
    """Ng = 65537, Nc = 3, Nb = 2, R = 2: the entry point launches slabs of 65535 genes.  Genes 65534..65536 against a call on those
    three alone, row 1 against its own call, and every pair solved."""
    Nc, Ng = 3, 65537
    rng = np.random.default_rng(5)
    p = BC.problem(rng.poisson(2.0, (Nc, Ng)) + 1.0, np.array([0.1, 2.0, 4.0]), np.array([1.0, 2.0, 3.0]), np.array([0, 0, 1]), 0, "Poisson")
    Wt = np.array([[1.0, 0.0, 2.0], [2.0, 1.0, 1.0]])
    st = stage(p)
    whole = launch(st, Wt)
    assert set(np.unique(whole["st"])) <= set(DONE) and np.isfinite(whole["nu"]).all() and np.isfinite(whole["dvar"]).all()
    three = launch(st, Wt, 65534, 65537)
    same({k: whole[k][:, 65534:] for k in NAMES}, three, "across the slab boundary")
    row1 = launch(st, Wt[1:])
    same({k: whole[k][1:] for k in NAMES}, row1, "row 1")


def test_cell_weights_of_the_worker():
    p = BC.cases()["seven_1_NegativeBinomial"]
    same_fit(run(p), run(p, cell_weights=np.ones(961)))
    p = BC.cases()["nu_prior"]
    same_fit(run(p), run(p, cell_weights=np.ones(300), chunk_genes=3))


def test_the_weights_are_permuted_with_the_cells():
    """The interleaved problem with a caller's 4-row table equals, bit for bit, the same problem handed over sorted by
    `batch_segments`' permutation with the table's columns permuted alike.  Both replicates start from the same full-data fit."""
    p, Wt = Q.cases()["interleaved"]
    assert (np.diff(p["labels"]) < 0).any()
    perm, _ = batch_segments(p["labels"], 3)
    q = BC.problem(p["S"][perm], p["phis"][perm], p["n"][perm], p["labels"][perm], p["H"], p["noisemodel"], p["dispersion"])
    fit = run(p)
    a, b = boot(p, weights=Wt, fit=fit, return_weights=True), boot(q, weights=Wt[:, perm], fit=fit, return_weights=True)
    same_boot(a, b)
    assert np.array_equal(a.weights, Wt.astype(np.float32)) and np.array_equal(b.weights, Wt[:, perm].astype(np.float32))
    assert not np.array_equal(a.replicates, boot(q, weights=Wt, fit=fit).replicates)          # the unpermuted table is another resample
    # and the one-row worker
    for w in Wt[:2]:
        x, y = run(p, cell_weights=w), run(q, cell_weights=w[perm])
        same_fit(x, y)


def test_drawn_weights():
    name = "seven_1_NegativeBinomial"
    p = BC.cases()[name]
    fit = run(p)
    b8 = boot(p, n_boot=8, seed=3, fit=fit, return_weights=True)
    assert b8.fit is fit and b8.replicates.shape == (8, 3, 5) and b8.delta_replicates.shape == (8, 7, 5)
    assert b8.status.shape == b8.iterations.shape == (8, 5)
    b4 = boot(p, n_boot=4, seed=3, fit=fit, return_weights=True)
    same_boot(b8, b4, slice(0, 4))
    assert b8.weights[:4].tobytes() == b4.weights.tobytes()
    same_boot(b8, boot(p, n_boot=8, seed=3, fit=fit, chunk_genes=2))
    same_boot(b8, boot(p, counts=sp.csr_matrix(p["S"].astype(np.float32)), n_boot=8, seed=3, fit=fit, storage="f32"))
    w = b8.weights
    assert w.dtype == np.float32 and w.tobytes() == draw_weights(8, 961, 3, torch.device("cuda")).cpu().numpy().tobytes()
    assert boot(p, n_boot=2, seed=3, fit=fit).weights is None
    # the worker is one call of the entry point on that table (in the caller's cell order), warm-started from the fit
    direct = launch(stage(p), w, start=(np.ascontiguousarray(fit.means.T), np.ascontiguousarray(fit.delta_nu.T)), want_var=False)
    assert np.array_equal(direct["nu"].transpose(0, 2, 1), b8.replicates) and np.array_equal(direct["delta"].transpose(0, 2, 1), b8.delta_replicates)
    assert np.array_equal(direct["st"], b8.status) and np.array_equal(direct["it"], b8.iterations)
    assert np.array_equal(boot(p, weights=w, fit=fit).replicates, b8.replicates)          # and the same table handed over
    auto = boot(p, n_boot=2, seed=3)                                                      # fit=None runs the unweighted fit first
    same_fit(auto.fit, fit)
    same_boot(b8, auto, slice(0, 2))
    assert (b8.n_ok == 8).all() and np.isfinite(b8.stds).all() and np.isfinite(b8.delta_nu_stds).all()


def test_containers():
    """`Cycle.from_phases_batch_mle(bootstrap=16)` on the round trip (600 x 30, three batches): the means are the plain call's, the stds
    the bootstrap's, and the bootstrap stds of nu and of delta_nu agree with those of the float64 reference replicates on the same table.

    The bound.  Replicate r of coefficient i differs from its float64 fit by e_r with |e_r| <= sqrt(e' H e) sqrt((H^-1)_ii)
    <= bar_coef std64_ri (Cauchy-Schwarz; std64_ri the float64 Hessian std of that replicate).  The ddof-1 standard deviation over the
    R replicates is a seminorm, so |std(x + e) - std(x)| <= std(e) <= sqrt(R / (R - 1)) max_r |e_r|.  Hence
    |std_dev_i - std_64_i| <= sqrt(R / (R - 1)) bar_coef max_r std64_ri, per coefficient and gene."""
    sim = BC.round_trip()
    S = sim["S"].astype(np.float32)
    Nc, Ng = S.shape
    obs = pd.DataFrame({"n_scounts": sim["n"]}, index=[f"c{i}" for i in range(Nc)])
    ph = Phases.from_array(G.directions(sim["phis"]), cell_names=list(obs.index))
    ad = AnnDataLite(S, S, obs=obs.copy())
    design = BC.one_hot(sim["labels"]).T
    cyc, fit = Cycle.from_phases_batch_mle(ph, ad, design, 1, 1, "NegativeBinomial", 0.3, return_fit=True, bootstrap=16, bootstrap_seed=5)
    cyc0, fit0 = Cycle.from_phases_batch_mle(ph, ad, design, 1, 1, "NegativeBinomial", 0.3, return_fit=True)
    assert fit0.bootstrap is None and "bootstrap" not in [f.name for f in fields(fit)]
    same_fit(fit, fit0)
    assert cyc.means.equals(cyc0.means) and not cyc.stds.equals(cyc0.stds)
    bs = fit.bootstrap
    assert bs.replicates.shape == (16, 3, 30) and bs.delta_replicates.shape == (16, 3, 30) and bs.fit is fit
    assert np.array_equal(cyc.stds.values, Cycle.from_array(fit.means, bs.stds, gene_names=cyc.means.columns).stds.values)
    assert np.array_equal(cyc0.stds.values, Cycle.from_array(fit.means, fit.stds, gene_names=cyc.means.columns).stds.values)
    p = BC.problem(sim["S"], sim["phis"], sim["n"], sim["labels"], 1, "NegativeBinomial", 0.3)
    ref = boot(p, n_boot=16, seed=5, fit=fit0, return_weights=True)
    same_boot(bs, ref)
    with pytest.raises(ValueError, match="dispersion"):
        Cycle.from_phases_batch_mle(ph, ad, design, 1, 1, "NegativeBinomial", "mle", bootstrap=4)
    with pytest.raises(ValueError, match="bootstrap"):
        Cycle.from_phases_batch_mle(ph, ad, design, bootstrap=-1)
    assert (bs.n_ok == 16).all()
    R, bar = 16, Q.bars()["coef"]
    B, logm = G.basis64(sim["phis"], 1), np.log(sim["n"])
    worst = 0.0
    for g in range(Ng):
        fits64 = [Q.reference64(np.trunc(sim["S"][:, g]), B, sim["labels"], logm, w.astype(np.float64), "NegativeBinomial", 1 / 0.3, None,
                                BC.DELTA_PRIOR) for w in ref.weights]
        assert all(f["status"] == G.CONVERGED for f in fits64)
        std64 = np.std(np.array([f["nu"] for f in fits64]), axis=0, ddof=1)
        bound = np.sqrt(R / (R - 1)) * bar * np.max(np.array([f["std"] for f in fits64]), axis=0)
        err = np.abs(np.concatenate([bs.stds[:, g], bs.delta_nu_stds[:, g]]) - std64)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (g, err, bound)
    print(f"bootstrap stds against the float64 replicates: worst {worst:.3g} of the bound")


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(noise=_lib.NOISE["Lognormal"])) == _lib.VC_ERR_UNSUPPORTED
    assert b"Lognormal" in lib.vc_last_error(None)
    for kw, msg in REFUSALS:
        assert lib.vc_gene_glm_batch_weighted(*batch_boot_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    torch.cuda.synchronize()                                      # nothing was launched: nothing can have faulted
