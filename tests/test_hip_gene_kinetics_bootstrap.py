"""GPU: the weighted kinetics fit (vc_gene_kinetics_weighted), `gene_kinetics(cell_weights=)`, `velocity_map(cell_weights=)`,
`velocity_map_bootstrap` and `AngularSpeed.from_kinetics_mle(bootstrap=)`, judged by tests/gene_kinetics_boot_checker.py: the float64 fit
of the cell-expanded data, with bars that are 4 x the float32 restatement's own distance from it
(tests/test_gene_kinetics_bootstrap_cpu.py asserts the checker's own conditions).  Every test prints the figures it asserts on."""
import ctypes as C
from dataclasses import fields
from functools import lru_cache

import numpy as np
import pandas as pd
import pytest
import torch
from scipy.special import gammaln

from tests import gene_kinetics_boot_checker as KB
from tests import gene_kinetics_checker as Q
from tests.test_gene_kinetics_bootstrap_cpu import ORDER, REFUSALS, kinw_args
from velocycle_amd import _lib
from velocycle_amd.anndata_lite import AnnDataLite
from velocycle_amd.containers import AngularSpeed, Cycle, Phases
from velocycle_amd.gene_bootstrap import draw_weights
from velocycle_amd.gene_harmonics import _stage
from velocycle_amd.gene_kinetics import GeneKineticsFit, check_arguments, gene_kinetics, omega_design, velocity_map
from velocycle_amd.kinetics_bootstrap import velocity_map_bootstrap

pytestmark = pytest.mark.gpu
NAMES = ("xy", "cov", "ll", "dec", "it", "st", "nc", "score", "info")
INTS = ("it", "st", "nc")
GUARD = 5
PATTERN = {torch.float64: -1234.5, torch.int32: -77}
DOCUMENTED = (Q.CONVERGED, Q.ROUNDING, Q.MAX_ITER, Q.UNBOUNDED)


# ---------------------------------------------------------------------------------------------------------------- helpers
def inputs(p, genes=slice(None)):
    disp = 1.0 / p["r"][genes] if p["r"] is not None else 0.3
    return (p["U"][:, genes].astype(np.float32), Q.directions(p["phis"]), p["n"], p["nu"][genes].T), \
        dict(noisemodel=p["noisemodel"], dispersion=disp)


def design_kw(p):
    return dict(harmonics_w=p["Hw"], condition_design=p["D"])


def fit_rows(p, Wt, **kw):
    """`gene_kinetics` of a problem at its own angular speed under the rows of weights Wt."""
    args, nb = inputs(p)
    return gene_kinetics(*args, nu_omega=p["nuw"], **design_kw(p), **nb, cell_weights=Wt, **kw)


def stage(p, storage="auto"):
    """The device inputs of a problem, staged as the workers stage them."""
    (U, xy, n, means), nb = inputs(p)
    basis, logm, nu, r, pr, _ = check_arguments(U, xy, n, means, 1, nb["noisemodel"], nb["dispersion"])
    dev = torch.device("cuda")
    Nc, Ng = U.shape
    _, kblk, kind = _stage(U, 0, Ng, Nc, dev, storage)
    f32 = lambda t: torch.as_tensor(t).to(torch.float32).to(dev).contiguous() if t is not None else None          # noqa: E731
    W = f32(omega_design(xy, p["Hw"], p["D"]))
    return dict(kblk=kblk, kind=kind, B=f32(basis), logm=f32(logm), nu=torch.as_tensor(nu).to(dev).contiguous(), W=W, r=f32(r),
                prior=torch.as_tensor(pr).to(dev).contiguous(), Nc=Nc, Ng=Ng, K=basis.shape[0], NW=int(W.shape[0]),
                noise=_lib.NOISE[nb["noisemodel"]], nuw=np.asarray(p["nuw"], dtype=np.float64))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() if a is not None else None


def _guarded(n, dtype):
    return torch.full((n + 2 * GUARD,), PATTERN[dtype], dtype=dtype, device="cuda")


def launch(st, weights=None, g0=0, g1=None, nuw=None, start=None, nu_rows=None, want_cov=True, tol=1e-10, max_iter=25, w_ptr=None,
           wstride=None, R=None):
    """One call of vc_gene_kinetics (weights and w_ptr None) or vc_gene_kinetics_weighted on genes [g0, g1): host arrays by name with
    the row axis in front.  nuw: [NW] shared or [R, NW]; start: [Ng, 2] shared or [R, Ng, 2]; nu_rows: [R, Ng, K] -- the per-row tables
    are handed over whole, advanced to gene g0, with the stride of the whole table.  Every output lies between guard bands of a fixed
    pattern, which must be intact afterwards."""
    lib = _lib.load()
    g1 = st["Ng"] if g1 is None else g1
    n, K, NW, Ng = g1 - g0, st["K"], st["NW"], st["Ng"]
    NWH = NW * (NW + 1) // 2
    weighted = weights is not None or w_ptr is not None
    if weights is not None:
        w_d = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).cuda()
        w_ptr, wstride, R = _ptr(w_d), st["Nc"], w_d.shape[0]
    R = R or 1
    sizes = dict(xy=(2, torch.float64), cov=(3, torch.float64), ll=(1, torch.float64), dec=(1, torch.float64), it=(1, torch.int32),
                 st=(1, torch.int32), nc=(1, torch.int32), score=(NW, torch.float64), info=(NWH, torch.float64))
    bufs = {k: _guarded(R * n * sizes[k][0], sizes[k][1]) for k in NAMES}
    outs = [C.c_void_p(bufs[k].data_ptr() + GUARD * bufs[k].element_size()) if (want_cov or k != "cov") else None for k in NAMES]
    nuw_d = _dev64(st["nuw"] if nuw is None else nuw)
    start_d, nu_d = _dev64(start), _dev64(nu_rows)
    at = lambda t, off: C.c_void_p(t.data_ptr() + 8 * off)                                       # noqa: E731
    sl = lambda t: t[g0:g1] if t is not None else None                                            # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = [_ptr(st["kblk"][g0:g1]), st["kind"], n, st["Nc"], st["Nc"], _ptr(st["B"]), K, _ptr(st["logm"])]
    if not weighted:
        assert nu_rows is None and nuw_d.ndim == 1 and (start_d is None or start_d.ndim == 2)
        rc = lib.vc_gene_kinetics(*head, _ptr(sl(st["nu"])), _ptr(st["W"]), NW, _ptr(nuw_d), st["noise"], _ptr(sl(st["r"])),
                                  _ptr(sl(st["prior"])), _ptr(sl(start_d)), float(tol), int(max_iter), *outs, stream)
    else:
        nu_p, nu_s = (_ptr(sl(st["nu"])), 0) if nu_d is None else (at(nu_d, g0 * K), Ng * K)
        st_p, st_s = (None, 0) if start_d is None else ((_ptr(sl(start_d)), 0) if start_d.ndim == 2 else (at(start_d, g0 * 2), Ng * 2))
        rc = lib.vc_gene_kinetics_weighted(*head, nu_p, nu_s, _ptr(st["W"]), NW, _ptr(nuw_d), NW if nuw_d.ndim == 2 else 0, st["noise"],
                                           _ptr(sl(st["r"])), _ptr(sl(st["prior"])), w_ptr, R, wstride, st_p, st_s, float(tol),
                                           int(max_iter), *outs, stream)
    assert rc == _lib.VC_OK, lib.vc_last_error(None)
    torch.cuda.synchronize()
    got = {}
    for k in NAMES:
        host = bufs[k].cpu().numpy()
        assert (host[:GUARD] == PATTERN[sizes[k][1]]).all() and (host[-GUARD:] == PATTERN[sizes[k][1]]).all(), f"guard band of {k}"
        body = host[GUARD:-GUARD]
        if k == "cov" and not want_cov:
            assert (body == PATTERN[torch.float64]).all(), "cov_dev NULL: nothing may be stored"
        got[k] = body.reshape(R, n, sizes[k][0]) if k not in ("ll", "dec") + INTS else body.reshape(R, n)
    return got


def same(a, b, what="", names=NAMES):
    for k in names:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def cat(parts, axis):
    return {k: np.concatenate([x[k] for x in parts], axis=axis) for k in NAMES}


def same_fit(a, b):
    for f in fields(GeneKineticsFit):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f.name


def same_map(a, b):
    same_fit(a.kinetics, b.kinetics)
    assert a.nu_omega.tobytes() == b.nu_omega.tobytes() and a.stds.tobytes() == b.stds.tobytes() and a.cov.tobytes() == b.cov.tobytes()
    assert (a.F, a.dec, a.rounds, a.status, a.n_excluded) == (b.F, b.dec, b.rounds, b.status, b.n_excluded)
    assert np.array_equal(a.included, b.included)


def host_const(p, w, g):
    """What the kernel's objective leaves out of the weighted log-likelihood of gene g, at the float32 r it reads."""
    k = p["U"][:, g]
    t = -gammaln(k + 1)
    if p["r"] is not None:
        r = float(np.float32(p["r"][g]))
        t = t + gammaln(k + r) - gammaln(r)
    return float((np.asarray(w) * t).sum())


def cov2(c):
    return np.array([[c[0], c[1]], [c[1], c[2]]])


def is_no_data(got, b, g):
    return (got["st"][b, g] == Q.NO_DATA and got["it"][b, g] == 0 and got["nc"][b, g] == 0 and
            all(np.isnan(got[k][b, g]).all() for k in ("xy", "cov", "ll", "dec", "score", "info")))


@lru_cache(maxsize=None)
def warm_start(name):
    """[Ng, 2]: the bootstrap's start of a case, the unweighted fit of its problem."""
    p = Q.cases()[name]
    args, nb = inputs(p)
    fit = gene_kinetics(*args, nu_omega=p["nuw"], **design_kw(p), **nb)
    return np.ascontiguousarray(np.stack([fit.log_gamma, fit.log_beta], 1))


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("name", KB.PAIR_CASES)
def test_bars(name):
    p, Wt, solved, bars = Q.cases()[name], KB.weights(name), KB.solved(name), KB.bars()
    R, Ng = Wt.shape[0], p["U"].shape[1]
    fit = fit_rows(p, Wt)                                             # the worker: loglik with the weighted constants
    assert fit.log_gamma.shape == (R, Ng) and fit.cov.shape == (R, Ng, 2, 2) and fit.stds.shape == (R, 2, Ng)
    assert fit.score_w.shape == (R, Ng, p["W"].shape[0]) and fit.info_w.shape == (R, Ng, p["W"].shape[0], p["W"].shape[0])
    key = "loglik_large" if name in Q.LARGE_CASES else "loglik"
    worst = dict(xy=0.0, cov=0.0, loglik=0.0, info=0.0, score=0.0)
    storages = ("u16", "f32") if p["U"].max() <= 65535 else ("f32",)
    first = None
    for storage in storages:
        st = stage(p, storage)
        for start in (None, warm_start(name)):
            got = launch(st, Wt, start=start)
            if start is None:
                first = first or got
                same(first, got, storage)                             # the other storage: the same bits
                assert got["xy"][:, :, 0].tobytes() == fit.log_gamma.tobytes() and np.array_equal(got["st"], fit.status)
            for b in range(R):
                for g in range(Ng):
                    s = solved[b][g]
                    if s is None:
                        assert is_no_data(got, b, g) and np.isnan(fit.loglik[b, g]), (name, b, g)
                        continue
                    f64 = s[0]
                    assert got["st"][b, g] in Q.INTERIOR and got["nc"][b, g] == 0, (name, storage, start is not None, b, g, got["st"][b, g])
                    assert got["it"][b, g] <= KB.iteration_bound(s, warm=start is not None), (name, b, g, got["it"][b, g])
                    worst["xy"] = max(worst["xy"], Q.xy_distance(got["xy"][b, g, 0], got["xy"][b, g, 1], f64))
                    worst["cov"] = max(worst["cov"], Q.sym_distance(cov2(got["cov"][b, g]), f64["inv"]))
                    worst["loglik"] = max(worst["loglik"], Q.loglik_distance(got["ll"][b, g] + host_const(p, Wt[b], g), f64))
                    if name in Q.SCORE_CASES:
                        NW = st["NW"]
                        info = np.zeros((NW, NW))
                        info[np.tril_indices(NW)] = got["info"][b, g]
                        worst["info"] = max(worst["info"], Q.sym_distance(info + np.tril(info, -1).T, f64["info"]))
    for b in range(R):                                                # the worker's log-likelihood is the kernel's plus the host constants
        for g in range(Ng):
            if solved[b][g] is not None:                              # (both float64 sums of Nc terms; at large counts they cancel against L)
                const = host_const(p, Wt[b], g)
                assert abs(fit.loglik[b, g] - (first["ll"][b, g] + const)) <= 1e-12 * max(solved[b][g][0]["abs"], abs(const))
                assert np.array_equal(fit.stds[b, :, g], np.sqrt(np.diag(fit.cov[b, g])))
    if name in Q.SCORE_CASES:                                         # the score at the SAME point: evaluate-only at the reference's optimum
        at = np.array([[[s[0]["x"], s[0]["y"]] for s in row] for row in solved])
        ev = launch(stage(p), Wt, start=at, max_iter=0)
        assert (ev["st"] == Q.EVALUATED).all() and ev["xy"].tobytes() == at.tobytes()
        for b in range(R):
            for g in range(Ng):
                worst["score"] = max(worst["score"], Q.score_distance(ev["score"][b, g], solved[b][g][0]))
    print(f"{name}: worst (x, y) {worst['xy']:.3g} se (bar {bars['xy']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), objective "
          f"{worst['loglik']:.3g} (bar {bars[key]:.3g}), information {worst['info']:.3g} (bar {bars['info']:.3g}), score {worst['score']:.3g} "
          f"(bar {bars['score']:.3g})")
    assert worst["xy"] <= bars["xy"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars[key]
    assert worst["info"] <= bars["info"] and worst["score"] <= bars["score"]


@pytest.mark.parametrize("name", [f"shape_{Nc}_{Ng}_{H}_{noise}" for Nc, Ng, H, noise in Q.SHAPES] + Q.SCORE_CASES)
def test_unit_weights_are_the_unweighted_fit(name):
    """A table of ones, R = 1 and all strides 0: every one of the eleven outputs is vc_gene_kinetics' bit for bit -- from the default
    start, from a given start, and evaluate-only."""
    p = Q.cases()[name]
    Nc = p["U"].shape[0]
    ones = np.ones((1, Nc))
    for storage in ("u16", "f32"):
        st = stage(p, storage)
        plain = launch(st)
        same(plain, launch(st, ones), storage)
        at = np.where(np.isfinite(plain["xy"][0]), plain["xy"][0], 0.0) + 0.05
        same(launch(st, start=at), launch(st, ones, start=at), "start")
        same(launch(st, start=at, max_iter=0), launch(st, ones, start=at, max_iter=0), "evaluate-only")
        same(launch(st, max_iter=2), launch(st, ones, max_iter=2), "max_iter")
    args, nb = inputs(p)
    kw = dict(nu_omega=p["nuw"], **design_kw(p), **nb)
    same_fit(gene_kinetics(*args, **kw), gene_kinetics(*args, **kw, cell_weights=np.ones(Nc)))


@pytest.mark.parametrize("name", ["score_257_5_2", "shape_65_4_2_Poisson"])
def test_rows_and_cuts(name):
    p, Wt = Q.cases()[name], KB.weights(name)
    Nc, Ng = p["U"].shape
    R = Wt.shape[0]
    st = stage(p, "u16")
    whole = launch(st, Wt)
    same(whole, launch(st, Wt), "repetition")
    same(whole, launch(stage(p, "f32"), Wt), "storage")
    same(whole, cat([launch(st, Wt[b:b + 1]) for b in range(R)], 0), "rows")
    same(whole, cat([launch(st, Wt, g, g + 1) for g in range(Ng)], 1), "genes")
    warm = warm_start(name)
    whole_w = launch(st, Wt, start=warm)
    same(whole_w, cat([launch(st, Wt, g, g + 1, start=warm) for g in range(Ng)], 1), "warm genes")
    assert whole_w["xy"].tobytes() != whole["xy"].tobytes()
    without = launch(st, Wt, want_cov=False)                          # cov_dev NULL changes nothing else
    same(whole, without, "cov NULL", [k for k in NAMES if k != "cov"])
    # a stride of Nc + 3 with NaN padding, the table advanced inside a larger one
    big = np.full((R + 2, Nc + 3), np.nan, dtype=np.float32)
    big[1:R + 1, :Nc] = Wt
    big_d = torch.from_numpy(big).cuda()
    same(whole, launch(st, None, R=R, w_ptr=C.c_void_p(big_d.data_ptr() + 4 * (Nc + 3)), wstride=Nc + 3), "stride")
    # the worker: chunks of genes, the storage and a vector of weights are rows and cuts of the same call
    ref = fit_rows(p, Wt)
    for extra in (dict(chunk_genes=1), dict(chunk_genes=2), dict(storage="f32")):
        same_fit(ref, fit_rows(p, Wt, **extra))
    one = fit_rows(p, Wt[1])
    for f in fields(GeneKineticsFit):
        assert getattr(one, f.name).tobytes() == getattr(ref, f.name)[1].tobytes(), f.name


def test_per_row_cycle_speed_and_start():
    """Row b of a call with per-row nu, nuw and start equals the call on that row alone with that row's tables shared, bit for bit;
    cut into genes the per-row tables are read at their own stride.  The per-row cycles are held to the checker."""
    name = KB.NU_ROWS_CASE
    p, Wt = Q.cases()[name], KB.weights(name)
    R, Ng = Wt.shape[0], p["U"].shape[1]
    st = stage(p)
    nus = KB.nu_rows(name, R)
    nuws = np.stack([p["nuw"] * (1.0 + 0.05 * b) for b in range(R)])
    starts = np.stack([warm_start(name) + 0.01 * b for b in range(R)])
    whole = launch(st, Wt, nuw=nuws, start=starts, nu_rows=nus)
    rows = []
    for b in range(R):
        alone = dict(st, nu=torch.from_numpy(np.ascontiguousarray(nus[b])).cuda(), nuw=nuws[b])
        rows.append(launch(alone, Wt[b:b + 1], start=starts[b]))
    same(whole, cat(rows, 0), "rows")
    same(whole, cat([launch(st, Wt, g0, g1, nuw=nuws, start=starts, nu_rows=nus) for g0, g1 in ((0, 2), (2, 3), (3, Ng))], 1), "genes")
    assert len({whole["xy"][b].tobytes() for b in range(R)}) == R
    # one per-row table at a time, the others shared
    same(launch(st, Wt, nu_rows=nus), cat([launch(dict(st, nu=torch.from_numpy(np.ascontiguousarray(nus[b])).cuda()), Wt[b:b + 1])
                                           for b in range(R)], 0), "nu only")
    same(launch(st, Wt, nuw=nuws), cat([launch(st, Wt[b:b + 1], nuw=nuws[b]) for b in range(R)], 0), "nuw only")
    same(launch(st, Wt, start=starts), cat([launch(st, Wt[b:b + 1], start=starts[b]) for b in range(R)], 0), "start only")
    # against the checker: row b at its own cycle, from the default and the warm start
    bars, worst = KB.bars(), dict(xy=0.0, cov=0.0)
    args, nb = inputs(p)
    fit = gene_kinetics(*args, nu_omega=p["nuw"], **design_kw(p), **nb, cell_weights=Wt, means_replicates=nus.transpose(0, 2, 1))
    direct = launch(st, Wt, nu_rows=nus)
    assert fit.log_gamma.tobytes() == direct["xy"][:, :, 0].tobytes() and fit.log_beta.tobytes() == direct["xy"][:, :, 1].tobytes()
    for got, warm in ((direct, False), (launch(st, Wt, nu_rows=nus, start=warm_start(name)), True)):
        for b, row in enumerate(KB.solved_nu_rows()):
            for g, s in enumerate(row):
                assert got["st"][b, g] in Q.INTERIOR and got["it"][b, g] <= KB.iteration_bound(s, warm)
                worst["xy"] = max(worst["xy"], Q.xy_distance(got["xy"][b, g, 0], got["xy"][b, g, 1], s[0]))
                worst["cov"] = max(worst["cov"], Q.sym_distance(cov2(got["cov"][b, g]), s[0]["inv"]))
    print(f"per-row cycles: worst (x, y) {worst['xy']:.3g} se (bar {bars['xy']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g})")
    assert worst["xy"] <= bars["xy"] and worst["cov"] <= bars["cov"]


def test_more_genes_than_one_launch_holds():
    """The entry point launches slabs of 65535 genes (the second grid dimension): a call over 65537 genes equals its cuts at the slab
    boundary and elsewhere bit for bit, every pair ends with a documented status at a finite point, the row of ones is
    vc_gene_kinetics' answer beyond the first slab too, and the worker goes through the same call."""
    Nc, Ng = 3, 65535 + 2
    rng = np.random.default_rng(5)
    phis = np.array([0.1, 2.0, 4.0])
    nu = np.stack([rng.uniform(1.0, 2.0, Ng), rng.uniform(-0.3, 0.3, Ng), rng.uniform(-0.3, 0.3, Ng)], 1)
    p = dict(U=rng.poisson(2.0, (Nc, Ng)) + 1.0, phis=phis, n=np.array([1.0, 2.0, 3.0]), nu=nu, W=Q.design64(phis), nuw=np.array([0.4]), r=None,
             noisemodel="Poisson", D=None, H=1, Hw=0, Nx=1)
    Wt = np.array([[1.0, 0.0, 2.0], [1.0, 1.0, 1.0]])
    st = stage(p)
    whole = launch(st, Wt)
    assert np.isin(whole["st"], DOCUMENTED).all() and all(np.isfinite(whole[k]).all() for k in NAMES)
    print("statuses:", np.unique(whole["st"], return_counts=True))
    for cut in (65535, 40000):
        same(whole, cat([launch(st, Wt, 0, cut), launch(st, Wt, cut, Ng)], 1), cut)
    one = launch(st)
    for k in NAMES:
        assert whole[k][1].tobytes() == one[k][0].tobytes(), k
    fit = fit_rows(p, Wt)
    assert fit.log_gamma.tobytes() == whole["xy"][:, :, 0].tobytes() and np.array_equal(fit.status, whole["st"])


def test_planted_rows():
    name = "shape_257_5_1_NegativeBinomial"
    p = Q.cases()[name]
    Nc, Ng = p["U"].shape
    cell = int(np.argmax(p["U"].min(1)))                              # the cell whose smallest count is largest
    Wt = np.ones((5, Nc), dtype=np.float32)
    Wt[1] = 0.0
    Wt[2, 100] = np.nan
    Wt[3] = 0.0
    Wt[3, cell] = 2.0
    st = stage(p)
    got = launch(st, Wt)
    same({k: got[k][[0, 4]] for k in NAMES}, cat([launch(st)] * 2, 0), "the neighbours of the planted rows")
    assert all(is_no_data(got, b, g) for b in (1, 2) for g in range(Ng))
    warm = launch(st, Wt, start=warm_start(name))                     # whatever start_dev holds
    assert all(is_no_data(warm, b, g) for b in (1, 2) for g in range(Ng))
    assert set(warm["st"][0]) <= set(Q.INTERIOR) and warm["xy"][0].tobytes() == warm["xy"][4].tobytes()
    for g in range(Ng):                                               # weight on a single cell: a fit where that cell has a count
        if p["U"][cell, g] > 0:
            assert got["st"][3, g] in DOCUMENTED and all(np.isfinite(got[k][3, g]).all() for k in NAMES), (g, got["st"][3, g])
        else:
            assert is_no_data(got, 3, g)
    assert (p["U"][cell] > 0).any()
    print("single cell:", got["st"][3], got["xy"][3].tolist())
    # an infinite weight is no data either (sum wt k is not a finite number)
    Wt[2, 100] = np.inf
    assert all(is_no_data(launch(st, Wt[2:3]), 0, g) for g in range(Ng))
    # a start that is not finite: NO_DATA for that (row, gene) alone
    bad = np.stack([warm_start(name)] * 2)
    bad[1, 2, 0] = np.nan
    mixed = launch(st, Wt[[0, 4]], start=bad)
    assert is_no_data(mixed, 1, 2) and mixed["xy"][0].tobytes() == warm["xy"][0].tobytes()
    assert np.delete(mixed["xy"][1], 2, 0).tobytes() == np.delete(warm["xy"][0], 2, 0).tobytes()


def test_evaluate_only_under_weights():
    """The objective, the decrement and n_clamped at Q.EVALUATE_AT under the three rows of weights (the last point clamps cells);
    n_clamped is the float64 count of the cells with w > 0 and z <= 0 on the float32 tables."""
    name = Q.EVALUATE_CASE
    p, Wt, ev = Q.cases()[name], KB.weights(name), KB.evaluated()
    R, Ng = Wt.shape[0], p["U"].shape[1]
    st = stage(p)
    bars, worst, clamped = KB.bars(), dict(loglik=0.0, dec=0.0), 0
    f32 = lambda v: v.astype(np.float32).astype(np.float64)                        # noqa: E731
    for i in range(len(Q.EVALUATE_AT)):
        at = np.array([[ev[(b, i, g)][2] for g in range(Ng)] for b in range(R)])
        got = launch(st, Wt, start=at, max_iter=0)
        assert (got["st"] == Q.EVALUATED).all() and (got["it"] == 0).all() and got["xy"].tobytes() == at.tobytes()
        for b in range(R):
            for g in range(Ng):
                ref, r32, _ = ev[(b, i, g)]
                k, B, logm, nu, r = Q.gene_inputs(p, g)
                count = KB.weighted_point64(at[b, g, 0], at[b, g, 1], k, f32(B), f32(logm), nu, f32(p["W"]), p["nuw"], Wt[b],
                                            p["noisemodel"], r)["n_clamped"]
                d = dict(loglik=Q.loglik_distance(got["ll"][b, g] + host_const(p, Wt[b], g), ref), dec=Q.dec_distance(got["dec"][b, g], ref))
                worst = {key: max(worst[key], d[key]) for key in worst}
                assert got["nc"][b, g] == count <= r32["n_clamped"], (b, i, g, got["nc"][b, g], count, r32["n_clamped"])
                assert Q.sym_distance(cov2(got["cov"][b, g]), ref["inv"]) <= 1e-4
                clamped += count
    print(f"evaluate-only under weights: worst objective {worst['loglik']:.3g} (bar {bars['ev_loglik']:.3g}), decrement {worst['dec']:.3g} "
          f"(bar {bars['ev_dec']:.3g}), {clamped} clamped cells counted")
    assert clamped > 0 and worst["loglik"] <= bars["ev_loglik"] and worst["dec"] <= bars["ev_dec"]
    # the default start the kernel forms is the weighted one: one step from it lands where a step from the given start lands
    at0 = np.array([[ev[(b, 0, g)][2] for g in range(Ng)] for b in range(R)])
    own, given = launch(st, Wt, max_iter=1), launch(st, Wt, start=at0, max_iter=1)
    assert np.abs(own["xy"] - given["xy"]).max() <= 1e-6


@pytest.mark.parametrize("name", Q.KINK_CASES)
def test_kink_cases_under_weights(name):
    """10-20 % of the cells clamped, two resamples: finite outputs, a documented status, f no lower than at the start, and n_clamped
    the float64 count at the kernel's own point."""
    p, Wt = Q.cases()[name], KB.weights(name, 2)
    fit = fit_rows(p, Wt)
    Nc, Ng = p["U"].shape
    f32 = lambda v: v.astype(np.float32).astype(np.float64)                        # noqa: E731
    for b, w in enumerate(Wt):
        for g in range(Ng):
            k, B, logm, nu, r = Q.gene_inputs(p, g)
            tabs = (k, f32(B), f32(logm), nu, f32(p["W"]), p["nuw"], w)
            at = KB.weighted_point64(fit.log_gamma[b, g], fit.log_beta[b, g], *tabs, p["noisemodel"], r)
            x0, y0 = KB.weighted_start(*tabs)
            f0 = KB.weighted_point64(x0, y0, *tabs, p["noisemodel"], r)["f"]
            print(f"{name} row {b} gene {g}: status {fit.status[b, g]}, {fit.iterations[b, g]} steps, {fit.n_clamped[b, g]} clamped "
                  f"({at['n_clamped']}), min |z| {np.abs(at['z'][w > 0]).min():.3g}, f {at['f']:.8g} from {f0:.8g}")
            assert fit.status[b, g] in DOCUMENTED and at["f"] >= f0
            if np.abs(at["z"][w > 0]).min() >= 1e-9:                  # no resampled cell sits on the kink: the count is unambiguous
                assert fit.n_clamped[b, g] == at["n_clamped"]
    assert all(np.isfinite(getattr(fit, f.name)).all() for f in fields(fit))
    print(f"{name}: {fit.n_clamped.sum() / ((Wt > 0).sum() * Ng):.3f} of the resampled cells clamped")
    assert fit.n_clamped.sum() > 0


def test_non_integer_weights():
    """uniform(0, 3) float32 weights against the reference written out from the weighted formulas (no expansion exists)."""
    p, Wt = Q.cases()[KB.UNIFORM_CASE], KB.uniform_weights()
    bars, worst = KB.bars(), dict(xy=0.0, cov=0.0, loglik=0.0)
    st = stage(p)
    for start in (None, warm_start(KB.UNIFORM_CASE)):
        got = launch(st, Wt, start=start)
        for b, row in enumerate(KB.solved_uniform()):
            for g, f64 in enumerate(row):
                assert got["st"][b, g] in Q.INTERIOR and got["nc"][b, g] == 0 and got["it"][b, g] <= f64["iterations"] + 2
                worst["xy"] = max(worst["xy"], Q.xy_distance(got["xy"][b, g, 0], got["xy"][b, g, 1], f64))
                worst["cov"] = max(worst["cov"], Q.sym_distance(cov2(got["cov"][b, g]), f64["inv"]))
                worst["loglik"] = max(worst["loglik"], Q.loglik_distance(got["ll"][b, g] + host_const(p, Wt[b], g), f64))
    print(f"non-integer weights: worst (x, y) {worst['xy']:.3g} se (bar {bars['xy']:.3g}), inverse {worst['cov']:.3g} (bar {bars['cov']:.3g}), "
          f"objective {worst['loglik']:.3g} (bar {bars['loglik']:.3g})")
    assert worst["xy"] <= bars["xy"] and worst["cov"] <= bars["cov"] and worst["loglik"] <= bars["loglik"]
    fit = fit_rows(p, Wt)
    assert fit.log_gamma.tobytes() == launch(st, Wt)["xy"][:, :, 0].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the outer fit
@lru_cache(maxsize=None)
def full_fit(name):
    p = Q.cases()[name]
    args, nb = inputs(p)
    return velocity_map(*args, **design_kw(p), **nb)


def boot(name, **kw):
    p = Q.cases()[name]
    args, nb = inputs(p)
    return velocity_map_bootstrap(*args, **design_kw(p), **nb, **kw)


def same_boot(a, b, rows_a=slice(None), rows_b=slice(None)):
    for f in ("nu_omega_replicates", "status", "rounds", "n_excluded", "F", "dec", "log_gamma_replicates", "log_beta_replicates",
              "kinetics_status"):
        x, y = getattr(a, f)[rows_a], getattr(b, f)[rows_b]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_outer_bootstrap_against_the_expansion(name):
    p, Wt, ref, bars = Q.cases()[name], KB.weights(name, KB.OUTER_ROWS), KB.outer_solved(name), KB.bars()
    fit = full_fit(name)
    bs = boot(name, weights=Wt, fit=fit, keep_kinetics=True)
    assert bs.fit is fit and bs.nu_omega_replicates.shape == (KB.OUTER_ROWS, 2 * p["Hw"] + 1, p["Nx"]) and bs.weights is None
    assert bs.log_gamma_replicates.shape == bs.kinetics_status.shape == (KB.OUTER_ROWS, p["U"].shape[1])
    args, nb = inputs(p)
    for b, (m64, m32, _) in enumerate(ref):
        v = bs.nu_omega_replicates[b].T.reshape(-1)
        d = v - m64["nuw"]
        dist = float(np.sqrt(d @ m64["J"] @ d))
        one = velocity_map(*args, **design_kw(p), **nb, cell_weights=Wt[b])          # the same replicate from velocity_map's own start
        d1 = one.nu_omega.T.reshape(-1) - m64["nuw"]
        dist1 = float(np.sqrt(d1 @ m64["J"] @ d1))
        std = float(np.abs(one.stds.T.reshape(-1) / m64["std"] - 1).max())
        print(f"{name} row {b}: nuw {v}, {dist:.3g} se from the expansion's optimum (velocity_map(cell_weights=): {dist1:.3g}; bar "
              f"{bars['nuw']:.3g}), {bs.rounds[b]} rounds (restatement {m32['rounds']}), stds off by {std:.3g} (bar {bars['std']:.3g}), "
              f"status {bs.status[b]}, dec {bs.dec[b]:.3g}, {bs.n_excluded[b]} excluded")
        assert bs.status[b] == "CONVERGED" and bs.n_excluded[b] == 0 and bs.rounds[b] <= m32["rounds"] + 1
        assert dist <= bars["nuw"] and (bs.kinetics_status[b] <= Q.ROUNDING).all()
        # velocity_map(cell_weights=) starts at the prior mean, not where the bars' restatement starts: it is held to the replicate
        # of the bootstrap from that same start, bit for bit, and to what its stopping rule promises -- dec <= tol_outer = 1e-8 is
        # 1e-4 standard errors in the metric of its own J, the Fisher profile information, which the checker documents as up to a
        # fifth of the plain one in these cases: 1e-3 standard errors of the reference, and stds that move as far relatively
        cold = boot(name, weights=Wt[b:b + 1], fit=fit, warm_start=False, keep_kinetics=True)
        assert cold.nu_omega_replicates[0].tobytes() == one.nu_omega.tobytes() and cold.status[0] == one.status == "CONVERGED"
        assert (cold.F[0], cold.dec[0], cold.rounds[0], cold.n_excluded[0]) == (one.F, one.dec, one.rounds, one.n_excluded) and one.n_excluded == 0
        assert cold.log_gamma_replicates[0].tobytes() == one.kinetics.log_gamma.tobytes()
        assert dist1 <= 1e-3 and std <= 1e-3
    assert bs.ok.all() and np.isfinite(bs.stds).all()


def test_replicates_do_not_know_of_each_other():
    """Replicate b of a 3-row run equals its own 1-row run bit for bit, whatever the chunking and the storage."""
    name = "outer_1500_30"
    Wt, fit = KB.weights(name), full_fit(name)
    bs = boot(name, weights=Wt, fit=fit, keep_kinetics=True)
    print("rounds:", bs.rounds, "status:", bs.status)
    assert len(set(bs.rounds)) > 1 or len({r.tobytes() for r in bs.nu_omega_replicates}) == 3
    for b, extra in enumerate((dict(), dict(chunk_genes=7), dict(storage="f32", chunk_genes=16))):
        same_boot(bs, boot(name, weights=Wt[b:b + 1], fit=fit, keep_kinetics=True, **extra), slice(b, b + 1))
    same_boot(bs, boot(name, weights=Wt[::-1].copy(), fit=fit, keep_kinetics=True), slice(None), slice(None, None, -1))


@pytest.mark.parametrize("name", Q.OUTER_CASES)
def test_a_row_of_ones_is_velocity_map(name):
    p = Q.cases()[name]
    Nc = p["U"].shape[0]
    fit = full_fit(name)
    bs = boot(name, weights=np.ones((1, Nc)), fit=fit, warm_start=False, keep_kinetics=True)
    assert bs.nu_omega_replicates[0].tobytes() == fit.nu_omega.tobytes() and bs.status[0] == fit.status
    assert (bs.F[0], bs.dec[0], bs.rounds[0], bs.n_excluded[0]) == (fit.F, fit.dec, fit.rounds, fit.n_excluded)
    assert bs.log_gamma_replicates[0].tobytes() == fit.kinetics.log_gamma.tobytes()
    assert bs.log_beta_replicates[0].tobytes() == fit.kinetics.log_beta.tobytes() and np.array_equal(bs.kinetics_status[0], fit.kinetics.status)
    args, nb = inputs(p)
    same_map(fit, velocity_map(*args, **design_kw(p), **nb, cell_weights=np.ones(Nc)))
    warm = boot(name, weights=np.ones((1, Nc)), fit=fit)              # started at the optimum: it stays there
    print(f"{name}: warm-started at the fit: {warm.rounds[0]} rounds, moved by {np.abs(warm.nu_omega_replicates[0] - fit.nu_omega).max():.3g}")
    assert warm.status[0] == "CONVERGED" and warm.rounds[0] <= 1
    assert np.abs(warm.nu_omega_replicates[0] - fit.nu_omega).max() <= 1e-3 * fit.stds.min()


def test_drawn_weights():
    name = "outer_1500_30"
    p, fit = Q.cases()[name], full_fit(name)
    b4 = boot(name, n_boot=4, seed=3, fit=fit, keep_kinetics=True, return_weights=True)
    b2 = boot(name, n_boot=2, seed=3, fit=fit, keep_kinetics=True, return_weights=True, chunk_genes=11)
    same_boot(b4, b2, slice(0, 2))
    w = b4.weights
    assert w.tobytes() == draw_weights(4, 1500, 3, torch.device("cuda")).cpu().numpy().tobytes() and b2.weights.tobytes() == w[:2].tobytes()
    assert w.dtype == np.float32 and w.shape == (4, 1500) and (w >= 0).all() and np.array_equal(w, np.round(w)) and 0.9 < w.mean() < 1.1
    same_boot(b4, boot(name, weights=w, fit=fit, keep_kinetics=True))            # the same table handed over
    other = boot(name, n_boot=4, seed=4, fit=fit)
    assert not np.array_equal(other.nu_omega_replicates, b4.nu_omega_replicates) and other.weights is None and other.log_gamma_replicates is None
    auto = boot(name, n_boot=2, seed=3)                               # fit=None runs velocity_map first
    same_map(auto.fit, fit)
    assert auto.nu_omega_replicates.tobytes() == b2.nu_omega_replicates.tobytes()
    assert b4.ok.all() and np.isfinite(b4.contrast(0, 1)).all() and b4.contrast_std(0, 1) > 0
    print(f"4 drawn replicates: ln(omega_0 / omega_1) {b4.contrast(0, 1)}, se {b4.contrast_std(0, 1):.3g}")


def test_a_gene_emptied_in_one_replicate_is_excluded_there_only():
    name = "outer_1500_30"
    p = Q.cases()[name]
    (U, xy, n, means), nb = inputs(p)
    g, some = 3, 60
    U = U.copy()
    U[some:, g] = 0                                                   # the gene's counts sit in the first 60 cells
    fit = velocity_map(U, xy, n, means, **design_kw(p), **nb)
    assert fit.status == "CONVERGED" and fit.included[g]
    Wt = np.ones((3, 1500))
    Wt[1, :some] = 0.0                                                # row 1 resamples none of them
    bs = velocity_map_bootstrap(U, xy, n, means, **design_kw(p), **nb, weights=Wt, fit=fit, keep_kinetics=True)
    print("excluded:", bs.n_excluded, "status:", bs.status, "kernel status of the gene:", bs.kinetics_status[:, g])
    assert list(bs.n_excluded) == [0, 1, 0] and bs.kinetics_status[1, g] == Q.NO_DATA and np.isnan(bs.log_gamma_replicates[1, g])
    assert (bs.status == "CONVERGED").all() and np.isfinite(bs.nu_omega_replicates).all() and np.isfinite(bs.F).all()
    same_boot(bs, bs, slice(0, 1), slice(2, 3))
    # a gene the full fit left out stays out of every replicate
    left = velocity_map(U, xy, n, means, **design_kw(p), **nb)
    left.included = left.included.copy()
    left.included[5] = False
    out = velocity_map_bootstrap(U, xy, n, means, **design_kw(p), **nb, weights=Wt, fit=left)
    assert list(out.n_excluded) == [1, 2, 1] and (out.status == "CONVERGED").all()
    assert not np.array_equal(out.nu_omega_replicates[0], bs.nu_omega_replicates[0])


def test_means_replicates_against_the_checker():
    name = KB.NU_ROWS_OUTER
    p, Wt, ref, bars = Q.cases()[name], KB.weights(name, KB.OUTER_ROWS), KB.outer_solved(name, True), KB.bars()
    nus = KB.nu_rows(name, KB.OUTER_ROWS)
    rep = np.ascontiguousarray(nus.transpose(0, 2, 1))                # [R, K, Ng] like GeneHarmonicBootstrap.replicates
    fit = full_fit(name)
    bs = boot(name, weights=Wt, fit=fit, means_replicates=rep, keep_kinetics=True)
    for b, (m64, m32, _) in enumerate(ref):
        d = bs.nu_omega_replicates[b].T.reshape(-1) - m64["nuw"]
        dist = float(np.sqrt(d @ m64["J"] @ d))
        print(f"row {b} at its own cycle: {dist:.3g} se from the expansion's optimum (bar {bars['nuw']:.3g}), {bs.rounds[b]} rounds "
              f"(restatement {m32['rounds']}), status {bs.status[b]}")
        assert bs.status[b] == "CONVERGED" and bs.n_excluded[b] == 0 and dist <= bars["nuw"] and bs.rounds[b] <= m32["rounds"] + 1
    plain = boot(name, weights=Wt, fit=fit)
    assert not np.array_equal(plain.nu_omega_replicates, bs.nu_omega_replicates)
    same_boot(bs, boot(name, weights=Wt[1:], fit=fit, means_replicates=rep[1:], keep_kinetics=True, chunk_genes=7), slice(1, 2))
    bad = rep.copy()
    bad[1, 1, 4] = np.nan                                             # a replicate whose cycle of one gene is not finite
    out = boot(name, weights=Wt, fit=fit, means_replicates=bad, keep_kinetics=True)
    assert list(out.n_excluded) == [0, 1] and out.kinetics_status[1, 4] == Q.NO_DATA and (out.status == "CONVERGED").all()
    same_boot(out, bs, slice(0, 1), slice(0, 1))


def test_container_path():
    name = "outer_1500_30"
    p = Q.cases()[name]
    (U, xy, n, means), nb = inputs(p)
    Nc, Ng = U.shape
    obs = pd.DataFrame({"n_scounts": n}, index=[f"c{i}" for i in range(Nc)])
    ad = AnnDataLite(U * 3, U, gene_names=[f"g{i}" for i in range(Ng)], obs=obs)
    ph = Phases.from_array(xy, cell_names=list(obs.index))
    cyc = Cycle.from_array(means, np.ones_like(means), gene_names=list(ad.var.index))
    prior = AngularSpeed.trivial_prior(["ctl", "trt"], harmonics=0)
    out, fit = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], prior=prior, return_fit=True,
                                              bootstrap=4, bootstrap_seed=5)
    out0, fit0 = AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, p["D"], nb["noisemodel"], nb["dispersion"], prior=prior, return_fit=True)
    same_map(fit, fit0)
    assert fit0.bootstrap is None and out.means.equals(out0.means) and out.stds.equals(out0.stds)          # the Laplace stds stay
    bs = fit.bootstrap
    assert bs.fit is fit and bs.nu_omega_replicates.shape == (4, 1, 2) and bs.ok.all()
    ref = velocity_map_bootstrap(U, xy, n, means, **design_kw(p), **nb, n_boot=4, seed=5, fit=fit0, nuw_prior=prior)
    assert ref.nu_omega_replicates.tobytes() == bs.nu_omega_replicates.tobytes() and ref.F.tobytes() == bs.F.tobytes()
    lap = np.sqrt(fit.cov[0, 0] / fit.nu_omega[0, 0] ** 2 + fit.cov[1, 1] / fit.nu_omega[0, 1] ** 2
                  - 2 * fit.cov[0, 1] / (fit.nu_omega[0, 0] * fit.nu_omega[0, 1]))
    print(f"ln(omega_ctl / omega_trt): Laplace se {lap:.3g}, bootstrap se over 4 replicates {bs.contrast_std(0, 1):.3g}")
    with pytest.raises(ValueError, match="bootstrap must be"):
        AngularSpeed.from_kinetics_mle(cyc, ph, ad, 0, p["D"], prior=prior, bootstrap=-1)


def test_refusals_through_the_c_abi():
    """Each with its code and a message, before anything is launched: the pointers handed over are not device memory."""
    lib = _lib.load()
    torch.cuda.synchronize()
    for kw, msg in REFUSALS + ORDER:
        assert lib.vc_gene_kinetics_weighted(*kinw_args(**kw)) == _lib.VC_ERR_ARG and msg in lib.vc_last_error(None), kw
    assert lib.vc_gene_kinetics_weighted(*kinw_args(noise=2)) == _lib.VC_ERR_UNSUPPORTED
    torch.cuda.synchronize()                                          # nothing was launched: nothing can have faulted
    with pytest.raises(ValueError, match="n_boot"):
        boot("outer_1500_30", n_boot=0)
