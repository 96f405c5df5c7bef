"""Checker of the weighted batch-aware per-gene harmonic regression (vc_gene_glm_batch_weighted / gene_harmonics_batched with
cell_weights / gene_harmonics_batched_bootstrap).  Like tests/gene_boot_checker.py it holds no weighted formula for integer weights: a
fit under integer case weights IS the unweighted fit of the data with cell c repeated w_c times.  The float64 reference of a
(gene, row) pair is `gene_glm_checker.newton64` on the augmented design of `gene_batch_checker.augmented` with its columns repeated;
the float32 restatement is `gene_batch_checker.restate32` on the same expansion, from the default start and from the warm start (the
concatenated float64 fit of the unweighted data, through `gene_boot_checker._starting_at`).

The trap: `gene_batch_checker.augmented` infers Nb from `labels.max()`, so an expansion that empties the LAST batch would lose a
coefficient.  `reference64` therefore builds the augmented design from the unexpanded labels and repeats its columns, and
`restatement32` runs `restate32` inside `_with_batches(Nb)`, which hands `one_hot` the batch count.

Non-integer weights: `gene_boot_checker.weighted_newton64` on the augmented design.

Bars: `gene_glm_checker.SAFETY` x the restatement's own worst distance from float64 over all pairs and both starts, on
`gene_batch_checker.distances`' yardsticks (coef, std, dstd, loglik, lr); computed here, never typed in."""
from contextlib import contextmanager
from functools import lru_cache

import numpy as np

from tests import gene_batch_checker as BC
from tests import gene_boot_checker as W
from tests import gene_glm_checker as G

WEIGHT_SEED = 11
ROWS = 4
DRAWN = ("seven_0_Poisson", "seven_1_Poisson", "seven_1_NegativeBinomial", "seven_2_NegativeBinomial", "one_batch", "one_and_1000",
         "max_batches", "interleaved", "silent_batch", "large_u16_Poisson", "large_f32_NegativeBinomial", "nu_prior")
EMPTY_LAST = "interleaved_empty_last"          # one hand-made row: weight 0 on the whole of the last batch
UNIFORM = "interleaved_uniform"                # one uniform(0, 3) float32 row: no restatement
YARDSTICKS = BC.YARDSTICKS


@lru_cache(maxsize=None)
def cases():
    """name -> (problem of tests/gene_batch_checker.py, weights float64 [R, Nc])."""
    base = BC.cases()
    out = {}
    for name in DRAWN:
        Nc = base[name]["S"].shape[0]
        out[name] = (base[name], np.random.default_rng(WEIGHT_SEED).poisson(1, (ROWS, Nc)).astype(np.float64))
    p = base["interleaved"]
    Nc = p["S"].shape[0]
    w = np.random.default_rng(WEIGHT_SEED).poisson(1, (1, Nc)).astype(np.float64)
    w[0, p["labels"] == p["labels"].max()] = 0.0
    out[EMPTY_LAST] = (p, w)
    uniform = np.random.default_rng(WEIGHT_SEED).uniform(0, 3, (1, Nc)).astype(np.float32)       # the table is float32 by contract
    out[UNIFORM] = (p, uniform.astype(np.float64))
    return out


def is_integer(name):
    w = cases()[name][1]
    return bool(np.array_equal(w, np.round(w)))


def n_batches(p):
    return int(np.asarray(p["labels"]).max()) + 1


def emptied(name):
    """bool [R, Nb]: the batches a row leaves without a cell of positive weight."""
    p, Wt = cases()[name]
    return np.array([[not (w[p["labels"] == b] > 0).any() for b in range(n_batches(p))] for w in Wt])


def reps_of(w):
    w = np.asarray(w)
    reps = w.astype(np.int64)
    assert np.array_equal(reps, w), "integer weights only"
    return reps


@contextmanager
def _with_batches(Nb):
    """`gene_batch_checker.restate32` builds its design from the labels it is given and asks `one_hot` without a batch count.  Within
    this block `one_hot` is told Nb, so that the restatement of an expansion that lost its last batch keeps all Nb offsets."""
    default = BC.one_hot
    BC.one_hot = lambda labels, _Nb=None: default(labels, Nb)
    try:
        yield
    finally:
        BC.one_hot = default


def reference64(k, B, labels, logm, w, noisemodel, r, prior, dprior):
    """The float64 fit of one gene under the weights w: newton64 on the expansion for integer weights, the written-out weighted Newton
    otherwise.  Over the K + Nb coefficients, nu first."""
    Ba, pa = BC.augmented(B, labels, prior, dprior)                                  # from the unexpanded labels: all Nb rows
    if np.array_equal(w, np.round(w)):
        reps = reps_of(w)
        out = G.newton64(np.repeat(k, reps), np.repeat(Ba, reps, axis=1), np.repeat(logm, reps), noisemodel, r, pa)
    else:
        out = W.weighted_newton64(k, Ba, logm, w, noisemodel, r, pa)
    out["K"] = B.shape[0]
    return out


def written_out64(k, B, labels, logm, w, noisemodel, r, prior, dprior):
    Ba, pa = BC.augmented(B, labels, prior, dprior)
    out = W.weighted_newton64(k, Ba, logm, np.asarray(w, dtype=np.float64), noisemodel, r, pa)
    out["K"] = B.shape[0]
    return out


def restatement32(k, B, labels, logm, w, noisemodel, r, prior, dprior, start=None):
    """gene_batch_checker.restate32 on the expansion; start: the K + Nb numbers it begins at (None: its default start)."""
    reps = reps_of(w)
    args = (np.repeat(k, reps), np.repeat(B, reps, axis=1), np.repeat(labels, reps), np.repeat(logm, reps), noisemodel, r, prior, dprior)
    with _with_batches(int(np.asarray(labels).max()) + 1):
        if start is None:
            return BC.restate32(*args)
        with W._starting_at(start):
            return BC.restate32(*args)


@lru_cache(maxsize=None)
def unweighted64(name):
    """Per gene: the float64 fit of the unweighted data over the K + Nb coefficients -- the warm start."""
    p = cases()[name][0]
    out = []
    for g in range(p["S"].shape[1]):
        k, B, lab, logm, r, prior, dprior = BC.gene_inputs(p, g)
        out.append(BC.newton64(k, B, lab, logm, p["noisemodel"], r, prior, dprior))
    return out


@lru_cache(maxsize=None)
def solved(name):
    """[row][gene] of a case: (float64 fit, float64 null fit, float32 restatement from the default start, its null, the restatement
    warm-started from the float64 fit of the unweighted data; the null model -- K = 1 with the offsets -- is never warm-started); the
    restatements are None under non-integer weights."""
    p, Wt = cases()[name]
    noise = p["noisemodel"]
    out = []
    for w in Wt:
        row = []
        for g in range(p["S"].shape[1]):
            k, B, lab, logm, r, prior, dprior = BC.gene_inputs(p, g)
            _, B0, _, _, _, prior0, _ = BC.gene_inputs(p, g, 0)
            f64 = reference64(k, B, lab, logm, w, noise, r, prior, dprior)
            n64 = reference64(k, B0, lab, logm, w, noise, r, prior0, dprior)
            if is_integer(name):
                row.append((f64, n64, restatement32(k, B, lab, logm, w, noise, r, prior, dprior),
                            restatement32(k, B0, lab, logm, w, noise, r, prior0, dprior),
                            restatement32(k, B, lab, logm, w, noise, r, prior, dprior, start=unweighted64(name)[g]["nu"])))
            else:
                row.append((f64, n64, None, None, None))
        out.append(row)
    return out


def bearing(name):
    """bool [R, Ng]: the pairs held to the bars (their float64 reference, and its null model, end CONVERGED)."""
    return np.array([[s[0]["status"] == G.CONVERGED and s[1]["status"] == G.CONVERGED for s in row] for row in solved(name)])


def left_out_share():
    keep = np.concatenate([bearing(name).reshape(-1) for name in cases()])
    return float((~keep).sum()) / keep.size


def restatement_distances(f64, n64, f32, n32):
    K = f64["K"]
    return BC.distances(f32["nu"][:K], f32["nu"][K:], f32["std"][:K], f32["std"][K:], f32["loglik"], 2 * (f32["loglik"] - n32["loglik"]),
                        f64, n64)


@lru_cache(maxsize=None)
def bars():
    """SAFETY x the restatement's worst distance from float64 over every pair of every integer-weight case, from both starts the GPU
    test runs (see gene_boot_checker.bars for why the warm start matters to the stds)."""
    worst = dict.fromkeys(YARDSTICKS, 0.0)
    for name in cases():
        if not is_integer(name):
            continue
        keep = bearing(name)
        for b, row in enumerate(solved(name)):
            for g, (f64, n64, f32, n32, f32w) in enumerate(row):
                if keep[b, g]:
                    for f in (f32, f32w):
                        d = restatement_distances(f64, n64, f, n32)
                        for key in worst:
                            worst[key] = max(worst[key], d[key])
    return {key: G.SAFETY * v for key, v in worst.items()}


def iteration_bound(name, b, g, warm=False):
    """The steps a device fit of the pair may take: the restatement's from the same start + 2; under non-integer weights (no
    restatement) the float64 Newton's + 2."""
    f64, _, f32, _, f32w = solved(name)[b][g]
    return ((f32w if warm else f32) if f32 is not None else f64)["iterations"] + 2
