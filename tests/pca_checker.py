"""Float64 checker of the PCA phase prior (Phases.from_pca_heuristic(device=...), velocycle_amd/phase_prior.py) and the checks
that tests/test_pca_prior_cpu.py (device="cpu") and tests/test_hip_pca_prior.py (device="cuda") share.

Fixtures: simulate_counts(Nc, Ng, seed)["S"], size-normalised to the mean total, small_count = 1.  Ragged in both dimensions, one with
fewer than 64 genes; their third-to-second singular-value ratios are 0.88-0.98 (the power iteration close to its hardest case).
Oracle: np.linalg.svd of the centred log(float64(v) + small_count); every component's entry of largest magnitude positive (the first
one on ties); the percentile normalisation of the host path.
Bar on the normalised scores: SAFETY x the error, against the same oracle, of the existing host path with PCA(svd_solver="full") on the
float32 log matrix (the project's usual margin over a float32 reference's own error; it covers the different summation order).
"""
import warnings
from functools import lru_cache

import numpy as np
import torch

FIXTURES = [(3000, 200, 0), (1500, 97, 1), (517, 65, 2), (200, 33, 3)]
SMALL = 1.0
SAFETY = 4.0
MIN_RADIUS = 0.05                    # below it the angle of a cell is ill-conditioned
MAX_LEFT_OUT = 0.03
EPS32 = float(np.finfo(np.float32).eps)


@lru_cache(maxsize=None)
def layer(i):
    """The size-normalised spliced layer of fixture i: float32 (Nc, Ng), read-only."""
    from velocycle_amd.simulate import simulate_counts
    Nc, Ng, seed = FIXTURES[i]
    S = simulate_counts(Nc, Ng, seed=seed)["S"].numpy().astype(np.float64)
    tot = np.maximum(S.sum(1), 1.0)
    v = (S / tot[:, None] * tot.mean()).astype(np.float32)
    v.setflags(write=False)
    return v


def adata(v, **kw):
    from velocycle_amd.anndata_lite import AnnDataLite
    ad = AnnDataLite(v, v, **kw)
    ad.layers["S_sz"] = v
    return ad


def normalise(pcs):
    lo, hi, med = np.percentile(pcs, [0.5, 99.5, 50], 0)
    return (pcs - med) / (hi - lo)


def flip(components):
    """rows = components: the entry of largest magnitude of every row positive (np.argmax: the first of equal ones)"""
    top = np.abs(components).argmax(1)
    s = np.sign(components[np.arange(components.shape[0]), top])
    s[s == 0] = 1.0
    return components * s[:, None]


@lru_cache(maxsize=None)
def oracle(i, n=2):
    """dict: components (n, Ng), pcs (Nc, n), norm (normalised pcs), angle, radius, singular values -- all float64"""
    X = np.log(layer(i).astype(np.float64) + SMALL)
    Xc = X - X.mean(0)
    _, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    comp = flip(Vt[:n])
    pcs = Xc @ comp.T
    norm = normalise(pcs)
    return dict(components=comp, pcs=pcs, norm=norm, angle=np.arctan2(norm[:, 1], norm[:, 0]) % (2 * np.pi),
                radius=np.hypot(norm[:, 0], norm[:, 1]), s=s, mean=X.mean(0))


@lru_cache(maxsize=None)
def host_full(i):
    """The existing host path with the exact solver on the float32 log matrix: (sklearn object, normalised pcs)."""
    from sklearn.decomposition import PCA
    X = np.log(layer(i) + np.float32(SMALL))
    assert X.dtype == np.float32
    pca = PCA(2, svd_solver="full")
    return pca, normalise(pca.fit_transform(X))


@lru_cache(maxsize=None)
def bar(i):
    return SAFETY * float(np.abs(host_full(i)[1] - oracle(i)["norm"]).max())


def angle_bar(i):
    return np.sqrt(2.0) * bar(i) / MIN_RADIUS


def circ(a, b):
    d = np.abs(a - b) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


@lru_cache(maxsize=None)
def prior(i, device, **kw):
    """Phases.from_pca_heuristic(device=device) on fixture i (computed once per (fixture, device, arguments); do not modify)."""
    from velocycle_amd.containers import Phases
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the default run converges: no warning
        return Phases.from_pca_heuristic(adata(layer(i)), layer="S_sz", small_count=SMALL, device=device, **dict(kw))


# ---- the checks shared by the CPU and the GPU suite ------------------------------------------------------------------------------

def check_scores(i, device):
    p, o = prior(i, device), oracle(i)
    err = float(np.abs(p.pcs - o["norm"]).max())
    print(f"fixture {FIXTURES[i]} on {device}: normalised pcs off the oracle by {err:.3e}, bar {bar(i):.3e} "
          f"(host 'full' {bar(i) / SAFETY:.3e}); {p.pca.n_iter_} iterations, residual {p.pca.residual_:.2e}; s3/s2 = {o['s'][2] / o['s'][1]:.3f}")
    assert p.pca.converged_ and p.pca.residual_ <= 1e-6
    assert p.pcs.shape == o["norm"].shape
    assert p.pca.pcs.dtype == torch.float32 and p.pca.pcs.device.type == torch.device(device).type
    assert p.pca.components_.dtype == np.float64 and p.pca.components_.shape == o["components"].shape
    assert err <= bar(i), (err, bar(i))
    # the record: mean, variance
    assert np.allclose(p.pca.mean_, o["mean"], rtol=0, atol=4 * EPS32 * np.abs(o["mean"]).max())
    Nc = FIXTURES[i][0]
    assert np.allclose(p.pca.explained_variance_, o["s"][:2] ** 2 / (Nc - 1), rtol=1e-4)


def check_angles(i, device):
    p, o = prior(i, device), oracle(i)
    keep = o["radius"] >= MIN_RADIUS
    left_out = 1.0 - keep.mean()
    got = np.arctan2(p.phi_xy.values[1], p.phi_xy.values[0]) % (2 * np.pi)
    err = float(circ(got, o["angle"])[keep].max())
    print(f"fixture {FIXTURES[i]} on {device}: angle off by {err:.3e}, bar {angle_bar(i):.3e}; {100 * left_out:.1f} % of the cells left out")
    assert left_out <= MAX_LEFT_OUT, left_out
    assert err <= angle_bar(i), (err, angle_bar(i))
    assert np.allclose(np.hypot(*p.phi_xy.values), 1.0, atol=1e-6)


def check_signs(i, device):
    p = prior(i, device)
    ref = host_full(i)[0].components_
    got = p.pca.components_
    assert (np.sum(got * ref, 1) > 0).all(), np.sum(got * ref, 1)
    top = np.abs(got).argmax(1)
    assert (got[np.arange(2), top] > 0).all()


def min_density_case():
    """(fixture, oracle start cell) where zero_at_min_density is well posed: the two widest gaps of the oracle's sorted angles differ
    by more than twice the angle bar and the two cells at the widest gap are well-conditioned.  The first fixture that qualifies."""
    for i in range(len(FIXTURES)):
        o = oracle(i)
        order = np.argsort(o["angle"])
        gaps = np.diff(o["angle"][order])
        k = int(gaps.argmax())
        two = np.sort(gaps)[-2:]
        if two[1] - two[0] > 2 * angle_bar(i) and o["radius"][order[k]] >= MIN_RADIUS and o["radius"][order[k + 1]] >= MIN_RADIUS:
            return i, int(order[k + 1]), float(two[1] - two[0])
    raise AssertionError("no fixture has a well-separated widest gap: take other seeds")


def check_min_density(device):
    i, start, margin = min_density_case()
    p = prior(i, device, zero_at_min_density=True, concentration=3.0)
    got = np.arctan2(p.phi_xy.values[1], p.phi_xy.values[0]) % (2 * np.pi)
    print(f"zero_at_min_density on fixture {FIXTURES[i]}: oracle start cell {start}, gap margin {margin:.3e} > 2 x {angle_bar(i):.3e}")
    assert margin > 2 * angle_bar(i)
    assert p.phi_xy.values[0, start] == 3.0 and p.phi_xy.values[1, start] == 0.0, p.phi_xy.values[:, start]
    # the same rotation of everything else
    o = oracle(i)
    keep = o["radius"] >= MIN_RADIUS
    assert circ(got, (o["angle"] - o["angle"][start]) % (2 * np.pi))[keep].max() <= 2 * angle_bar(i)
    assert np.allclose(np.hypot(*p.phi_xy.values), 3.0, atol=1e-5)


def check_variants(device):
    """genes_to_use, CSR = dense bits, float64 layer, chunk_cells, repetition, max_iter, device=None."""
    import scipy.sparse as sp
    from velocycle_amd.containers import Phases
    from velocycle_amd.phase_prior import PCAScores, pca_scores
    i = 2                                                    # 517 x 65
    v = layer(i)
    Nc, Ng, _ = FIXTURES[i]
    base = prior(i, device)
    run = lambda lay, **kw: pca_scores(lay, SMALL, 2, device=device, **kw)
    same = lambda a, b: (torch.equal(a.pcs.cpu(), b.pcs.cpu()) and np.array_equal(a.components_, b.components_)
                         and np.array_equal(a.mean_, b.mean_) and a.n_iter_ == b.n_iter_ and a.residual_ == b.residual_)
    first = run(v)
    assert isinstance(first, PCAScores) and same(first, base.pca)
    assert same(first, run(v)), "repetition"
    for chunk in (64, 192, Nc):
        assert same(first, run(v, chunk_cells=chunk)), chunk
    assert same(first, run(sp.csr_matrix(v))) and same(first, run(sp.csc_matrix(v), chunk_cells=64)), "sparse"
    assert same(first, run(torch.from_numpy(v.copy())))
    f64 = run(v.astype(np.float64))                          # float32 values held as float64: the same staged matrix
    assert same(first, f64)
    # genes_to_use: the prior of the sub-matrix
    names = adata(v).var.index
    use = [g for k, g in enumerate(names) if k % 3 != 1]
    sub = Phases.from_pca_heuristic(adata(v), genes_to_use=use, layer="S_sz", small_count=SMALL, device=device)
    direct = run(np.ascontiguousarray(v[:, [k for k in range(Ng) if k % 3 != 1]]))
    assert sub.pca.components_.shape == (2, len(use)) and same(sub.pca, direct)
    # another start block: the same answer within the bar, not the same bits
    other = run(v, random_state=7)
    assert not same(first, other)
    assert np.abs(normalise(other.pcs.cpu().numpy().astype(np.float64)) - oracle(i)["norm"]).max() <= bar(i)
    # n_components = 3: the first two are the same directions
    three = pca_scores(v, SMALL, 3, device=device)
    assert three.pcs.shape == (Nc, 3) and three.components_.shape == (3, Ng)
    assert np.abs(np.sum(three.components_[:2] * oracle(i)["components"], 1)).min() > 1 - 1e-6
    # max_iter: a warning, not an exception
    import pytest
    with pytest.warns(RuntimeWarning, match="max_iter"):
        short = run(v, max_iter=2)
    assert short.converged_ is False and short.n_iter_ == 2 and short.residual_ > 1e-6 and short.pcs.shape == (Nc, 2)
    with pytest.warns(RuntimeWarning, match="max_iter"):
        p = Phases.from_pca_heuristic(adata(v), layer="S_sz", small_count=SMALL, device=device, max_iter=2)
    assert p.pca.converged_ is False and np.isfinite(p.phi_xy.values).all()


def check_refusals(device, monkeypatch):
    import pytest
    from velocycle_amd import phase_prior
    from velocycle_amd.containers import Phases
    v = layer(3)
    run = lambda lay, n=2, **kw: phase_prior.pca_scores(lay, SMALL, n, device=device, **kw)
    with pytest.raises(ValueError, match="n_components"):
        run(v, 5)
    with pytest.raises(ValueError, match="at least 8 genes"):
        run(v[:, :7])
    with pytest.raises(ValueError, match="at least 2 cells"):
        run(v[:1])
    with pytest.raises(ValueError, match="plot=True"):
        Phases.from_pca_heuristic(adata(v), layer="S_sz", small_count=SMALL, device=device, plot=True)
    with pytest.raises(ValueError, match="not a valid entry"):
        Phases.from_pca_heuristic(adata(v), layer="nope", device=device)
    # values the logarithm cannot take: raised after staging, nothing iterated
    calls = []
    for cls in (phase_prior._TorchOps, phase_prior._HipOps):
        monkeypatch.setattr(cls, "apply", lambda self, Q: calls.append(1))
    for badv in (-SMALL, -2.0, np.nan, np.inf):
        w = v.copy()
        w[150, 20] = badv
        with pytest.raises(ValueError, match="not finite"):
            run(w, chunk_cells=64)
    assert not calls
    monkeypatch.undo()
    # a matrix that does not fit
    monkeypatch.setattr(phase_prior, "_free_bytes", lambda dev: 4 * v.size)
    with pytest.raises(ValueError, match="free memory"):
        run(v)
