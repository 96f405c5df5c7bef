"""CPU: the layouts of tests/cabi_layouts.py are what they claim to be, so that tests/test_hip_cabi_layouts.py and
tests/test_hip_cabi_layouts_six.py are not vacuous: every layout holds the problem's matrix at g * gene_stride + c and poison (or
another seed's counts) everywhere else, the two mistakes they are there for change what every gene reads, the guard check sees a
single planted element, and the 32-bit row-index geometry keeps every truncated index inside its allocation and on poison.  For the
six later entry points (weights, per-row tables with a stride, a second count matrix, per-cell views) every further layout is held
the same way: the right index formula returns the table, and each mistake the layout is there for, restated as an index formula on
the host buffers, stays inside the buffer and reads NaN, poison or another row's numbers -- where the compact layout could not tell."""
from functools import lru_cache

import numpy as np
import pytest

from tests import cabi_layouts as L
from tests import gene_batch_checker as BC
from tests import gene_dispersion_checker as D
from tests import gene_glm_checker as G
from tests import gene_kinetics_checker as Q

STORAGES = ("u16", "f32")
KERNELS = ("glm", "batch", "dispersion", "kinetics", "mle", "glmw", "batchw", "kinw", "cell", "joint", "jointw")
WEIGHTED = ("glmw", "batchw", "kinw", "jointw")
JOINT = ("joint", "jointw")


@lru_cache(maxsize=None)
def spec(kernel, storage, tables="rows"):
    """One small problem per entry point, from the checkers, staged by the workers' own staging on the host."""
    if kernel == "glmw":
        from tests import gene_boot_checker as W
        p, Wt = W.cases()["shape_65_7_3_NegativeBinomial"]
        return L.glm_weighted_spec(p, L.case_weights(Wt), storage, warm=True)
    if kernel == "batchw":
        from tests import gene_batch_boot_checker as BW
        p, Wt = BW.cases()["silent_batch"]
        return L.batch_weighted_spec(p, L.case_weights(Wt), storage, warm=True)
    if kernel == "kinw":
        from tests import gene_kinetics_boot_checker as KB
        return L.kinetics_weighted_spec(Q.cases()["score_257_5_3"], L.case_weights(KB.weights("score_257_5_3")), storage, tables=tables)
    if kernel == "cell":
        from tests import cell_speed_checker as CS
        return L.cell_speed_spec(CS.cases()["shape_63_4_2_Poisson"], storage, varied=True)
    if kernel in JOINT:
        from tests import gene_joint_boot_checker as X
        from tests import gene_joint_checker as J
        p = J.cases()["score_257_5_3"]
        if kernel == "joint":
            return L.joint_spec(p, storage, start=True)
        return L.joint_weighted_spec(p, L.case_weights(X.weights("score_257_5_3")), storage, tables=tables)
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


# ----------------------------------------------------------------------------------------------- the six later entry points' layouts
def rowtabs(s):
    """(table, numbers per gene) of every per-row table of a spec."""
    return [(a[1], a[2]) for a in s["args"] if a[0] == "rowtab" and a[1] is not None]


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("kernel", JOINT)
def test_the_second_layer_stands_in_its_own_buffer_with_the_other_parity(kernel, storage):
    """Both layers in every layout: one gene_stride, U's matrix at its own base with poison (a window's left columns: a third seed's
    counts) around it, and under an odd padding every row of U on an element of the other parity than that row of S.  U read through S's
    base offset finds other numbers inside U's buffer; the compact layout cannot tell (both bases are 0)."""
    s = spec(kernel, storage)
    S, U = s["M"], s["M2"]
    Ng_all, Nc = S.shape
    assert U.shape == S.shape and U.dtype == S.dtype and not same(S, U)
    for lay in layouts(Ng_all):
        buf, base, stride, Ng = L.count_buffer(S, lay)
        buf2, base2, stride2, Ng2 = L.count_buffer(U, lay, second=True)
        g0, g1 = lay.genes if lay.genes is not None else (0, Ng_all)
        assert (stride2, Ng2) == (stride, Ng)
        idx = base2 + np.arange(Ng)[:, None] * stride + np.arange(Nc)[None, :]
        assert idx.max() < buf2.size and same(buf2[idx], U[g0:g1]), lay.name
        first = base2 - g0 * stride
        inside = np.zeros(buf2.size, dtype=bool)
        inside[first + np.arange(Ng_all)[:, None] * stride + np.arange(Nc)[None, :]] = True
        other = np.zeros(buf2.size, dtype=bool)
        if lay.left:
            cols = first - lay.left + np.arange(Ng_all)[:, None] * stride + np.arange(lay.left)[None, :]
            other[cols] = True
            assert same(buf2[cols], L.other_counts(U, lay.left, L.THIRD_SEED)) and not same(buf2[cols], L.other_counts(U, lay.left))
        assert L.is_poison(buf2[~inside & ~other]).all(), lay.name
        if lay is L.compact:
            assert (base, base2) == (0, 0) and buf2.size == U.size
            continue
        rows, rows2 = base + np.arange(Ng) * stride, base2 + np.arange(Ng) * stride
        assert ((rows + rows2) % 2 == 1).all(), lay.name                          # row g of S odd where row g of U is even, and back
        wrong = buf2[base + np.arange(Ng)[:, None] * stride + np.arange(Nc)[None, :]]          # U read through S's base offset
        assert base != base2 and not same(wrong, U[g0:g1]), lay.name
    p1 = L.padded(1)
    assert {L.count_buffer(S, p1)[1] % 2, L.count_buffer(U, p1, second=True)[1] % 2} == {0, 1}


@pytest.mark.parametrize("kernel", WEIGHTED)
def test_the_weight_layouts_hold_the_table_and_nan_between_its_rows(kernel):
    """weights_padded and row_range on the host buffer: w_bc at base + b * weight_stride + c and NaN everywhere else; b * Nc for
    b * weight_stride stays inside and reads a NaN in every row but the first; the row index dropped reads row 0's weights, which are
    not row b's; a row walked to its stride reads NaN.  The compact table cannot tell the first and the last: its stride is Nc."""
    Wt = L.weights_of(spec(kernel, "u16"))
    R_all, Nc = Wt.shape
    assert Wt.dtype == np.float32 and R_all == 3 and all(not same(Wt[0], Wt[b]) for b in range(1, R_all))
    assert (Wt[1] == 0).any() and (Wt[1] != np.round(Wt[1])).any() and np.isfinite(Wt).all() and (Wt >= 0).all()
    for lay in (L.weights_padded(1), L.weights_padded(61), L.both(L.row_range(1, 3), L.weights_padded(1)), L.row_range(1, 2)):
        buf, base, stride, R = L.weight_buffer(Wt, lay)
        b0, b1 = lay.rows if lay.rows is not None else (0, R_all)
        assert R == b1 - b0 and stride == Nc + lay.wpad and base == b0 * stride
        idx = base + np.arange(R)[:, None] * stride + np.arange(Nc)[None, :]
        assert idx.max() < buf.size and same(buf[idx], Wt[b0:b1]), lay.name
        inside = np.zeros(buf.size, dtype=bool)
        inside[np.arange(R_all)[:, None] * stride + np.arange(Nc)[None, :]] = True
        assert np.isnan(buf[~inside]).all() and (~inside).sum() == R_all * lay.wpad
        for b in range(1, R):
            assert not same(buf[base:base + Nc], Wt[b0 + b])                                  # the row index dropped
            if lay.wpad:
                wrong = buf[base + b * Nc:base + b * Nc + Nc]                                  # b * Nc for b * weight_stride
                assert wrong.size == Nc and np.isnan(wrong).any(), (lay.name, b)
        if lay.wpad:
            walked = buf[base:base + stride]
            assert walked.size == stride and np.isnan(walked[Nc:]).all()
    buf, base, stride, R = L.weight_buffer(Wt, L.compact)
    assert (base, stride, R) == (0, Nc, R_all) and same(buf.reshape(R_all, Nc), Wt)


@pytest.mark.parametrize("kernel", ["kinw", "jointw"])
def test_the_row_stride_layouts_hold_every_rows_table_and_nan_between_them(kernel):
    """row_strides, row_range and shared_tables on the host buffers of nu, nuw and start.  Entry i of row b's table stands at
    base + b * row_stride + i and NaN lies between the tables.  The mistakes, restated as index formulas: the table's width (NW, Ng K,
    2 Ng, Ng (K + 2)) for its stride, and the row index dropped, read inside the buffer and never row b's table; a stride of 0 taken as
    the table's width reads NaN behind the one shared table.  With the stride equal to the width (compact) the first cannot show."""
    s = spec(kernel, "u16")
    Ng, K, NW, R_all = s["M"].shape[0], s["K"], s["NW"], 3
    tabs = rowtabs(s)
    widths = [T.shape[1] for T, _ in tabs]
    assert widths == ([Ng * K, NW, 2 * Ng] if kernel == "kinw" else [NW, Ng * (K + 2)]) and all(T.shape[0] == R_all for T, _ in tabs)
    for T, per_gene in tabs:
        width = T.shape[1]
        assert np.isfinite(T).all() and all(not same(T[0], T[b]) for b in range(1, R_all))
        for lay in (L.row_strides(1), L.row_strides(7), L.both(L.row_range(1, 3), L.row_strides(1)), L.both(L.row_range(2, 3), L.row_strides(7))):
            buf, base, stride = L.row_table_buffer(T, lay, per_gene)
            b0, b1 = lay.rows if lay.rows is not None else (0, R_all)
            assert stride == width + lay.rpad and base == b0 * stride
            right = base + np.arange(b1 - b0)[:, None] * stride + np.arange(width)[None, :]
            assert right.max() < buf.size and same(buf[right], T[b0:b1]), lay.name
            inside = np.zeros(buf.size, dtype=bool)
            inside[np.arange(R_all)[:, None] * stride + np.arange(width)[None, :]] = True
            assert np.isnan(buf[~inside]).all() and (~inside).sum() == R_all * lay.rpad
            for b in range(1, b1 - b0):
                wrong = base + b * width + np.arange(width)                                    # the width for the stride
                assert wrong.max() < buf.size and (wrong != right[b]).all() and not same(buf[wrong], T[b0 + b]), (lay.name, b)
                assert (np.isnan(buf[wrong]) | inside[wrong]).all()                            # each a NaN, or a number of another table
                assert not same(buf[right[0]], T[b0 + b])                                      # the row index dropped
        # a gene range keeps the whole table's stride: row b of the view starts at g0 * per_gene + b * stride, not at b * (call's width)
        if per_gene:
            lay = L.gene_range(1, Ng - 1)
            buf, base, stride = L.row_table_buffer(T, lay, per_gene)
            n = (Ng - 2) * per_gene
            assert base == per_gene and stride == width >= n
            for b in range(R_all):
                assert same(buf[base + b * stride:base + b * stride + n], T[b].reshape(Ng, per_gene)[1:Ng - 1].reshape(-1))
                if b:
                    assert not same(buf[base + b * n:base + b * n + n], T[b].reshape(Ng, per_gene)[1:Ng - 1].reshape(-1))
        # the compact buffer: the stride is the width, so the width taken for the stride reads the right table
        buf, base, stride = L.row_table_buffer(T, L.compact, per_gene)
        assert (base, stride) == (0, width) and same(buf.reshape(R_all, width), T)
    copies = rowtabs(spec(kernel, "u16", "copies"))
    assert len(copies) == len(tabs)
    for (C, per_gene), (T, _) in zip(copies, tabs):
        assert C.shape == T.shape and all(same(C[b], T[0]) for b in range(R_all))
        buf, base, stride = L.row_table_buffer(C, L.shared_tables, per_gene)
        width = C.shape[1]
        assert (base, stride) == (0, 0) and same(buf[:width], T[0]) and buf.size == R_all * width
        for b in range(1, R_all):                                                            # a stride of 0 taken as the width
            assert np.isnan(buf[b * width:(b + 1) * width]).all()
    shared = rowtabs(spec(kernel, "u16", "shared"))
    assert all(T.ndim == 1 and L.row_table_buffer(T, L.compact, pg)[1:] == (0, 0) for T, pg in shared)


@pytest.mark.parametrize("width", [1, 3, 7, 28])
def test_a_gene_ranges_output_row_laid_out_with_the_whole_problems_genes_lands_in_the_band(width):
    """The weighted kernels store row b, gene g of a call at b * Ng_call + g.  In a gene range's own block [R][n], an index formed with
    the whole problem's Ng -- b * Ng_all + g -- stays inside the tensor, and from row 1 on it is not the right slot: it lands on another
    slot of the block (whose bytes then differ from the whole call's) or in the band behind it, which `bands_intact` then sees."""
    R, Ng_all = 3, 7
    for g0, g1 in ((1, Ng_all - 1), (1, 2)):
        n = g1 - g0
        whole, body = L.row_output_block(R, n, Ng_all, width, np.float64)
        assert body == R * n * width and L.bands_intact(whole, body)
        for b in range(R):
            for g in range(n):
                right, wrong = L.GUARD + (b * n + g) * width, L.GUARD + (b * Ng_all + g) * width
                assert wrong + width <= whole.size and (wrong == right) == (b == 0)
                if wrong >= L.GUARD + body:
                    w = whole.copy()
                    w[wrong] = 1.0
                    assert not L.bands_intact(w, body)
        assert L.GUARD + ((R - 1) * Ng_all + n - 1) * width >= L.GUARD + body                 # the last row does leave the block


@pytest.mark.parametrize("storage", STORAGES)
def test_a_cell_range_has_real_cells_either_side(storage):
    """cell_range on the host buffer: counts_dev advanced by c0 with the full width as gene_stride.  The call's cell c of gene g stands at
    base + g * Nc_all + c; a cell index without c0 stays inside, reads real counts, and not this range's; a row walked to gene_stride from
    counts_dev stays inside.  The per-cell tables (logm, prior, start) differ from cell to cell, so a view read without its offset shows."""
    s = spec("cell", storage)
    M = s["M"]
    Ng, Nc_all = M.shape
    for c0, c1 in ((1, 62), (5, 6), (37, 63)):
        lay = L.cell_range(c0, c1)
        buf, base, stride, n = L.count_buffer(M, lay)
        Nc = c1 - c0
        assert (base, stride, n) == (c0, Nc_all, Ng) and buf.size == M.size + c0
        idx = base + np.arange(Ng)[:, None] * stride + np.arange(Nc)[None, :]
        assert same(buf[idx], M[:, c0:c1])
        wrong = buf[idx - c0]
        assert not L.is_poison(wrong).any() and same(wrong, M[:, :Nc]) and (Nc == 1 or not same(wrong, M[:, c0:c1]))
        assert base + Ng * stride <= buf.size and L.is_poison(buf[M.size:]).all()
    percell = [a[1].numpy() for a in s["args"] if a[0] == "percell"]
    assert len(percell) == 3 and all(t.shape[0] == Nc_all for t in percell)
    for t in percell:
        assert len({t[c].tobytes() for c in range(Nc_all)}) == Nc_all


def test_truncated_indices_of_the_second_layer_and_of_the_weight_rows_stay_inside_and_on_poison():
    """Integers only, as for the first layer.  U's rows stand BIG_U_OFFSET elements behind S's in the same allocation and overlap
    neither S's rows nor each other; an index g * gene_stride + c kept in 32 bits addresses, through either base, an element of the
    allocation that is no row of either layer.  The weight table: b * weight_stride + c kept in 32 bits addresses a float of its own
    allocation that is no row of it."""
    assert L.BIG_U_OFFSET > L.BIG_NC and L.BIG_ALLOC == L.BIG_TOTAL + L.BIG_U_OFFSET and 2 * L.BIG_ALLOC < L.BIG_FREE_NEEDED
    rows = [(L.big_row_start(g, u), L.big_row_start(g, u) + L.BIG_NC) for g in range(L.BIG_NG) for u in (False, True)]
    rows.sort()
    assert rows[0][0] == L.BIG_BASE and rows[-1][1] == L.BIG_ALLOC and all(a[1] <= b[0] for a, b in zip(rows, rows[1:]))
    wrows = [(L.bigw_row_start(b), L.bigw_row_start(b) + L.BIG_NC) for b in range(L.BIGW_ROWS)]
    assert wrows[0][0] == L.BIG_BASE and wrows[-1][1] == L.BIGW_TOTAL and all(a[1] < b[0] for a, b in zip(wrows, wrows[1:]))
    assert 4 * L.BIGW_TOTAL < L.BIGW_FREE_NEEDED and 4 * L.BIGW_TOTAL + 2 * L.BIG_ALLOC > L.BIG_FREE_NEEDED     # why it has a rule of its own
    for base, total, taken in ((L.BIG_BASE, L.BIG_ALLOC, rows), (L.BIG_BASE + L.BIG_U_OFFSET, L.BIG_ALLOC, rows), (L.BIG_BASE, L.BIGW_TOTAL, wrows)):
        differs = dict(sign=set(), zero=set())
        for g in range(L.BIG_NG):
            for c in range(L.BIG_NC):
                true = g * L.BIG_STRIDE + c
                low = true % 2 ** 32
                for kind, idx in (("sign", low - 2 ** 32 if low >= 2 ** 31 else low), ("zero", low)):
                    at = base + idx
                    assert 0 <= at < total, (kind, g, c)
                    if idx != true:
                        differs[kind].add(g)
                        assert not any(a <= at < b for a, b in taken), (kind, g, c)
        assert differs["sign"] == {2} and differs["zero"] == set()
