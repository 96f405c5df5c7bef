"""CPU: the layouts of tests/cabi_layouts.py are what they claim to be, so that tests/test_hip_cabi_layouts.py is not vacuous: every
layout holds the problem's matrix at g * gene_stride + c and poison (or another seed's counts) everywhere else, the two mistakes they
are there for change what every gene reads, the guard check sees a single planted element, and the 32-bit row-index geometry keeps
every truncated index inside its allocation and on poison."""
from functools import lru_cache

import numpy as np
import pytest

from tests import cabi_layouts as L
from tests import gene_batch_checker as BC
from tests import gene_dispersion_checker as D
from tests import gene_glm_checker as G
from tests import gene_kinetics_checker as Q

STORAGES = ("u16", "f32")
KERNELS = ("glm", "batch", "dispersion", "kinetics", "mle")


@lru_cache(maxsize=None)
def spec(kernel, storage):
    """One small problem per entry point, from the checkers, staged by the workers' own staging on the host."""
    if kernel == "glm":
        return L.glm_spec(G.cases()["shape_65_7_3_NegativeBinomial"], storage)
    if kernel == "batch":
        return L.batch_spec(BC.cases()["silent_batch"], storage)
    if kernel == "dispersion":
        p = D.simulate(65, 7, 3)
        return L.dispersion_spec(dict(p, nu=p["nu_true"]), storage)
    if kernel == "kinetics":
        return L.kinetics_spec(Q.cases()["shape_65_4_2_Poisson"], storage)
    from tests.test_hip_cycle_mle import problem
    S, T, n = problem(63, 7, 33, seed=70)
    return L.mle_spec(S, T, n, "NegativeBinomial", 0.3, storage)


def layouts(Ng):
    return [L.compact, L.padded(1), L.padded(3), L.padded(61), L.window(5, 7), L.gene_range(1, Ng - 1), L.gene_range(1, 2)]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_every_layout_holds_the_matrix_and_poison_around_it(kernel, storage):
    M = spec(kernel, storage)["M"]
    Ng_all, Nc = M.shape
    assert M.dtype == (np.uint16 if storage == "u16" else np.float32) and Ng_all >= 4 and M.sum() > 0
    for lay in layouts(Ng_all):
        buf, base, stride, Ng = L.count_buffer(M, lay)
        g0, g1 = lay.genes if lay.genes is not None else (0, Ng_all)
        assert Ng == g1 - g0 and stride >= Nc and stride == lay.left + Nc + lay.pad + lay.right
        idx = base + np.arange(Ng)[:, None] * stride + np.arange(Nc)[None, :]
        assert idx.max() < buf.size and same(buf[idx], M[g0:g1]), lay.name
        # everything that is not a cell of the whole matrix: poison, or in a window's left columns the other seed's counts
        first = base - g0 * stride
        inside = np.zeros(buf.size, dtype=bool)
        inside[first + np.arange(Ng_all)[:, None] * stride + np.arange(Nc)[None, :]] = True
        other = np.zeros(buf.size, dtype=bool)
        if lay.left:
            cols = first - lay.left + np.arange(Ng_all)[:, None] * stride + np.arange(lay.left)[None, :]
            other[cols] = True
            assert same(buf[cols], L.other_counts(M, lay.left)) and not L.is_poison(buf[cols]).any()
        assert L.is_poison(buf[~inside & ~other]).all() and not (inside & other).any(), lay.name
        if lay is not L.compact:
            assert (~inside).sum() >= Ng_all * (stride - Nc) > 0
            assert L.is_poison(buf[idx[:, -1] + 1]).all()                          # the element after every row of the call
        # an odd padding is there for rows on odd elements: uint16 rows whose address is only 2-byte aligned
        if lay.pad % 2 == 1:
            rows = base + np.arange(Ng) * stride
            assert (rows % 2 == 1).any(), (lay.name, stride)
            if stride % 2 == 1 and Ng > 1:
                assert (rows % 2 == 0).any()
    assert L.count_buffer(M, L.compact)[1:3] == (0, Nc)
    assert L.count_buffer(M, L.window(5, 7))[1:3] == (5, Nc + 12)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_two_mistakes_change_what_every_gene_reads(kernel, storage):
    """A row base g * Nc, and a row walked to gene_stride, restated on the layouts' buffers: the counts a checker would be handed."""
    M = spec(kernel, storage)["M"]
    Ng_all, Nc = M.shape
    for lay in (L.padded(1), L.padded(3), L.padded(61), L.window(5, 7)):
        buf, base, stride, Ng = L.count_buffer(M, lay)
        for g in range(Ng):
            wrong_base = buf[base + g * Nc:base + g * Nc + Nc]
            assert wrong_base.size == Nc and (g == 0 or not same(wrong_base, M[g])), (lay.name, g)
            walked = buf[base + g * stride:base + (g + 1) * stride]
            assert walked.size == stride > Nc and same(walked[:Nc], M[g]), (lay.name, g)       # in bounds even for the last row
            extra = walked[Nc:]
            assert L.is_poison(extra[:1]).all() and L.is_poison(extra).sum() >= lay.pad + lay.right
            assert not (walked.astype(np.float64).sum() == M[g].astype(np.float64).sum()), (lay.name, g)
    # the compact layout cannot tell: both mistakes read the matrix itself
    buf, base, stride, Ng = L.count_buffer(M, L.compact)
    assert stride == Nc and same(buf.reshape(Ng, Nc), M)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32])
def test_the_guard_check_sees_one_planted_element(dtype):
    n = 10
    whole = L.guarded(n, dtype)
    assert whole.size == n + 2 * L.GUARD and L.bands_intact(whole) and L.untouched(whole)
    whole[L.GUARD:L.GUARD + n] = 1                                                  # the output itself
    assert L.bands_intact(whole) and not L.untouched(whole[L.GUARD:L.GUARD + n])
    for at in (L.GUARD - 1, L.GUARD + n, 0, whole.size - 1):
        w = whole.copy()
        w[at] = 1
        assert not L.bands_intact(w), at
    w = whole.copy()
    w.view(np.uint8)[L.GUARD * w.dtype.itemsize - 1] ^= 1                             # one bit of the last byte before the output
    assert not L.bands_intact(w)


def test_a_truncated_row_index_stays_inside_the_big_allocation_and_on_poison():
    """Integers only.  An index g * gene_stride + c kept in 32 bits, sign- or zero-extended, addresses an element of the allocation
    (counts_dev stands BIG_BASE elements into it), and wherever it is not the true index that element is poison, not a row."""
    assert L.BIG_STRIDE == 2 ** 30 + 1 and L.BIG_BASE == 2 ** 31 and (L.BIG_NG, L.BIG_NC) == (3, 257)
    assert L.BIG_TOTAL == 2 ** 31 + 2 * L.BIG_STRIDE + 257 and 2 * L.BIG_TOTAL < L.BIG_FREE_NEEDED == 12 * 10 ** 9
    rows = [(L.big_row_start(g), L.big_row_start(g) + L.BIG_NC) for g in range(L.BIG_NG)]
    assert rows[0][0] == L.BIG_BASE and rows[-1][1] == L.BIG_TOTAL and all(a[1] < b[0] for a, b in zip(rows, rows[1:]))
    differs = dict(sign=set(), zero=set())
    for g in range(L.BIG_NG):
        for c in range(L.BIG_NC):
            true = g * L.BIG_STRIDE + c
            low = true % 2 ** 32
            for kind, idx in (("sign", low - 2 ** 32 if low >= 2 ** 31 else low), ("zero", low)):
                at = L.BIG_BASE + idx                                               # relative to the allocation's base
                assert 0 <= at < L.BIG_TOTAL, (kind, g, c)
                if idx != true:
                    differs[kind].add(g)
                    assert not any(a <= at < b for a, b in rows), (kind, g, c)
    # a signed 32-bit product goes wrong at the last gene (2 gene_stride >= 2^31); an unsigned one is still right at three genes
    assert differs["sign"] == {2} and differs["zero"] == set()
