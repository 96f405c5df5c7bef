"""Yardstick of the SVI noise stream (csrc/vc_common.h: vc_philox_normal / vc_philox_normal2): a numpy
restatement of the standard-normal draw eps(seed, step, index) that shares nothing with the device code but the documented
layout, and the statistics that hold a stream of such draws to N(0, 1) and to independence.

normals() is the checker: the Philox4x32-10 block of tests/ppc_checker.py, the two 24-bit uniforms formed in float32 exactly as
the device forms them (one IEEE add, round to even: `n + 0.5` does NOT fit float32's significand for n >= 2^23, so u1 can round to
exactly 1.0 -- part of the specification), and everything after that in float64.  normals32() is "the reference's own error": the
same operations with one float32 rounding each, used only to report the scale of float32 rounding next to the device's error.
"""
import math
from statistics import NormalDist

import numpy as np

from tests.ppc_checker import philox

M32 = np.uint64(0xFFFFFFFF)
TOL = 1e-4                        # elementwise |device - normals()|: a wrong counter, key, index, branch or offset moves a draw by O(1)
BAR = 6.0                         # |z| of every goodness-of-fit / independence statistic
RAD_MAX = math.sqrt(50.0 * math.log(2.0))      # u1 = 2^-25, the smallest uniform: sqrt(-2 ln 2^-25) = 5.887
NBINS = 40
# the two rounding edges of the 24-bit uniform at index 0, found offline with this restatement (a vectorised search over the steps of
# seed 20240917); the CPU suite asserts what they are, the GPU suite runs the device there
EDGE_ONE = (20240917, 48605145)       # word 0 = 0xFFFFFFFC: (w >> 8) + 0.5 rounds to 2^24, u1 = 1.0 exactly, radius 0
EDGE_SMALL = (20240917, 8879789)      # word 0 = 0x000000B3: w >> 8 = 0, u1 = 2^-25, the largest radius sqrt(50 ln 2) = 5.887


def _u64(v):
    """Python int (any sign) -> its two's-complement uint64."""
    return int(v) & 0xFFFFFFFFFFFFFFFF


def words(seed, step, gidx):
    """The Philox block of each global index: counter (blk lo, blk hi, step lo, step hi), blk = gidx >> 1; key (seed lo, seed hi)."""
    gidx = np.asarray(gidx, dtype=np.uint64)
    blk = gidx >> np.uint64(1)
    step, seed = _u64(step), _u64(seed)
    return philox(blk & M32, blk >> np.uint64(32), np.uint64(step & 0xFFFFFFFF), np.uint64(step >> 32),
                  seed & 0xFFFFFFFF, seed >> 32)


def uniform24(w):
    """((float)(w >> 8) + 0.5f) * 2^-24 in float32: the conversion is exact, the add rounds to even, the scaling is exact."""
    return ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def radius(seed, step, gidx):
    """float64 Box-Muller radius sqrt(-2 ln u1) of each index's block."""
    u1 = uniform24(words(seed, step, gidx)[0]).astype(np.float64)
    return np.sqrt(-2.0 * math.log(2.0) * np.log2(u1))


def normals(seed, step, gidx):
    """float64 eps(seed, step, gidx): even index rad cos(2 pi u2), odd index rad sin(2 pi u2) of block gidx >> 1."""
    gidx = np.asarray(gidx, dtype=np.uint64)
    w = words(seed, step, gidx)
    u1 = uniform24(w[0]).astype(np.float64)
    u2 = uniform24(w[1]).astype(np.float64)
    rad = np.sqrt(-2.0 * math.log(2.0) * np.log2(u1))
    ang = 2.0 * math.pi * u2
    return rad * np.where((gidx & np.uint64(1)).astype(bool), np.sin(ang), np.cos(ang))


def normals32(seed, step, gidx):
    """normals() with every operation in numpy float32 (returned widened)."""
    f = np.float32
    gidx = np.asarray(gidx, dtype=np.uint64)
    w = words(seed, step, gidx)
    u1, u2 = uniform24(w[0]), uniform24(w[1])
    rad = np.sqrt((f(-2.0) * f(0.6931471805599453)) * np.log2(u1))
    ang = f(6.283185307179586) * u2
    out = rad * np.where((gidx & np.uint64(1)).astype(bool), np.sin(ang), np.cos(ang))
    assert out.dtype == np.float32
    return out.astype(np.float64)


def global_index(engine):
    """Local eps index -> the global index the counter takes: the identity below eps_n_global (the replicated sites); the ϕxy
    tail of a rank that starts at cell c0 is shifted by 2 c0."""
    idx = np.arange(engine.eps_total, dtype=np.int64)
    idx[engine.eps_n_global:] += 2 * int(engine.c0)
    return idx


def slot_names(engine):
    """Name of every local eps slot: its site, or "align" for a slot no site owns (the one alignment slot in front of ϕxy).
    Asserts that the slices are disjoint and cover [0, eps_total) apart from that slot."""
    names = np.full(engine.eps_total, "align", dtype=object)
    owned = np.zeros(engine.eps_total, dtype=np.int64)
    for n, (off, size) in engine.eps_slices.items():
        assert 0 <= off and off + size <= engine.eps_total, (n, off, size)
        names[off:off + size] = n
        owned[off:off + size] += 1
    assert owned.max() <= 1, "eps slices overlap"
    free = np.nonzero(owned == 0)[0]
    assert free.size <= 1 and (free.size == 0 or free[0] == engine.eps_n_global - 1), free
    assert engine.eps_slices["ϕxy"][0] == engine.eps_n_global and engine.eps_n_global % 2 == 0
    return names


_EDGES = np.array([NormalDist().inv_cdf(k / NBINS) for k in range(1, NBINS)])


def gof(x):
    """z-scores of a sample against N(0, 1): the first four raw moments (standard errors sqrt(1/n), sqrt(2/n), sqrt(15/n),
    sqrt(96/n)) and a chi-square on 40 equiprobable bins as (chi2 - 39) / sqrt(78)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    x2 = x * x
    cnt = np.bincount(np.searchsorted(_EDGES, x), minlength=NBINS)
    e = n / NBINS
    chi2 = float(((cnt - e) ** 2).sum() / e)
    return {"mean": float(x.mean() * math.sqrt(n)),
            "var": float((x2.mean() - 1.0) / math.sqrt(2.0 / n)),
            "m3": float((x2 * x).mean() / math.sqrt(15.0 / n)),
            "m4": float(((x2 * x2).mean() - 3.0) / math.sqrt(96.0 / n)),
            "chi2": (chi2 - (NBINS - 1)) / math.sqrt(2.0 * (NBINS - 1))}


def cross(x, y):
    """z of the correlation of two N(0, 1) samples: mean(x y) sqrt(n)."""
    x, y = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(y, dtype=np.float64).reshape(-1)
    return float((x * y).mean() * math.sqrt(x.size))


def cross_squares(a, b):
    """z of the correlation of the squares: mean((a^2 - 1)(b^2 - 1)) sqrt(n) / 2."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(((a * a - 1.0) * (b * b - 1.0)).mean() * math.sqrt(a.size) / 2.0)


def within(x, valid=None):
    """Independence inside one stream `x` of shape (streams, n) at consecutive global indices starting at an even one: the even
    vs the odd member of a pair, lag 1, lag 2, and the squares of the pair members.  `valid` (n,) masks slots out."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(-1, x.shape[-1])
    v = np.ones(x.shape[1], dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    m = x.shape[1] // 2 * 2
    pv = v[0:m:2] & v[1:m:2]
    a, b = x[:, 0:m:2][:, pv], x[:, 1:m:2][:, pv]
    l1, l2 = v[:-1] & v[1:], v[:-2] & v[2:]
    return {"pair": cross(a, b), "lag1": cross(x[:, :-1][:, l1], x[:, 1:][:, l1]),
            "lag2": cross(x[:, :-2][:, l2], x[:, 2:][:, l2]), "pair_squares": cross_squares(a, b)}
