"""Direct calls of the eleven engine-less entry points of include/velocycle_hip.h -- vc_gene_glm, vc_gene_glm_batch, vc_gene_dispersion,
vc_gene_kinetics, vc_phase_mle, vc_gene_glm_weighted, vc_gene_glm_batch_weighted, vc_gene_kinetics_weighted, vc_cell_speed, vc_gene_joint,
vc_gene_joint_weighted -- in every memory layout the header allows, not only the one the Python workers use.

A *spec* is one problem staged on the host by the workers' own staging (`check_arguments`, `fourier_basis_from_directions`, `_stage`'s
uint16 bits, `gene_batch`'s sort and segments, `phase_mle.stage_tables`, `check_weights`, `omega_design`): the count matrix as the
kernels read it, [genes][cells] (the joint kernels: two of them, S and U), and the entry point's argument list with a role per argument.
A *layout* says where those arrays stand in device memory.  `direct_call` makes ONE `lib.vc_*` call of a spec in a layout and returns
every output as a host array, with the state of the guard bands around them.

Layouts (what each one catches):
  compact            gene_stride == Nc, weight_stride == Nc, per-row tables exactly one table apart, fresh allocations: the workers'
                     convention
  padded(p)          the count block is [Ng][Nc + p], the padding poison (0xFFFF | NaN): a row base formed with Nc, a row walked to
                     gene_stride; odd p puts uint16 rows on addresses that are only 2-byte aligned (`count_buffer`).  The joint kernels'
                     second layer is a separate allocation with the other lead, so that where a row of S is odd-aligned that row of U is
                     even-aligned: a load path chosen from the alignment of one layer and used for both
  window(l, r)       the block is [Ng][l + Nc + r], counts_dev advanced by l, gene_stride the full width: the zero-copy way to cut cells;
                     the left columns hold counts of another seed (a neighbour's cell gives another number, not a NaN; U: a third
                     seed's), the right poison
  gene_range(a, b)   counts_dev at row a of the whole padded(3) block, every per-gene input and output the view at a of a whole-problem
                     tensor: the cut of the genes into calls; rows outside [a, b) of the outputs must keep their sentinel.  The weighted
                     kernels store row b of the weights at b * Ng_call + g: their outputs are an own guarded [R][b - a] block, and the
                     per-row per-gene tables (nu, start) are views at a with the whole table's row stride: an output row formed with the
                     whole problem's Ng, a table row formed with the call's width
  offset_inputs      every per-cell input is a view at an odd element of a larger NaN tensor: an alignment taken for granted
  side_stream        inputs produced and kernel launched on a fresh stream behind one large copy: a launch on another stream reads zeros
  big_stride         gene_stride = 2^30 + 1 with counts_dev 2^31 elements into an allocation filled with 0xFF: a row index formed in 32 bits
                     (the joint kernels: U's rows BIG_U_OFFSET elements behind S's in the same allocation)
  weights_padded(p)  the weight table is [R][Nc + p], what lies between NaN: b * Nc for b * weight_stride, a weight row walked to its stride
  row_strides(p)     every per-row table (nu, nuw, start) is [R][width + p], what lies between NaN: b * NW, b * Ng K, b * 2 Ng,
                     b * Ng (K + 2) for b * row_stride, or the row index dropped
  shared_tables      all row strides 0 and ONE table, held to the call whose R tables are R copies of it: a stride of 0 taken as non-zero
  row_range(a, b)    weights_dev advanced a * weight_stride, every per-row table a * stride, R = b - a, the outputs the view at row a of
                     whole-problem [R_all][Ng][...] tensors: "row b of an R-row call equals the call on that row alone"; rows outside
                     keep their sentinel
  cell_range(a, b)   vc_cell_speed: counts_dev advanced by a with the full width as gene_stride (a window with real cells either side),
                     logm, prior, start and the seven outputs views at a of whole-problem tensors, the basis re-packed [K][b - a]: a cell
                     index without the offset; cells outside keep their sentinel
  big_weight_stride  weight_stride = 2^30 + 1 with weights_dev 2^31 floats into an allocation filled with 0xFF (NaN): b * weight_stride
                     formed in 32 bits
In every layout every output lives inside a larger tensor with GUARD elements of a fixed bit pattern before and after it.

Importing this module needs no GPU: the buffers are built with numpy (tests/test_cabi_layouts_cpu.py checks them there)."""
import ctypes as C
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np
import torch

from tests import gene_glm_checker as G
from velocycle_amd import _lib
from velocycle_amd import cell_speed as CSP
from velocycle_amd import gene_batch as GB
from velocycle_amd import gene_harmonics as GH
from velocycle_amd import gene_joint as GJ
from velocycle_amd import gene_kinetics as GK
from velocycle_amd import phase_mle as PM

GUARD = 64                       # elements of the sentinel before and after every output
SENTINEL = 0xA5                  # every byte of a guard band, and of an output before the launch
POISON_U16 = 0xFFFF
ODD = 3                          # the element an offset input starts at
OTHER_SEED = 77                  # of the counts in a window's left columns
THIRD_SEED = 78                  # of the counts in the left columns of a window's second layer
BIG_STRIDE = (1 << 30) + 1
BIG_BASE = 1 << 31               # elements in front of counts_dev in the big allocation
BIG_NG, BIG_NC = 3, 257
BIG_TOTAL = BIG_BASE + (BIG_NG - 1) * BIG_STRIDE + BIG_NC          # uint16 elements: about 8.6 GB
BIG_U_OFFSET = 300               # the joint kernels' second layer: row g of U starts this many elements behind row g of S
BIG_ALLOC = BIG_TOTAL + BIG_U_OFFSET                               # what `big_allocation` holds
BIG_FREE_NEEDED = 12 * 10 ** 9     # bytes that must be free for the 32-bit row-index tests to run
BIGW_ROWS = 3
BIGW_TOTAL = BIG_BASE + (BIGW_ROWS - 1) * BIG_STRIDE + BIG_NC      # float32 elements: about 17.2 GB
BIGW_FREE_NEEDED = 24 * 10 ** 9    # the same rule for the weight table: 4 BIGW_TOTAL bytes in one allocation, and room for the rest
BALLAST_BYTES = 1 << 30          # the copy a side stream makes first: about a millisecond, a launch takes microseconds
CPU = torch.device("cpu")
TOL, MAX_ITER = 1e-10, 25        # the workers' defaults
JOINT_MAX_ITER = 40              # gene_joint's


@dataclass(frozen=True)
class Layout:
    name: str
    pad: int = 0
    left: int = 0
    right: int = 0
    genes: Optional[Tuple[int, int]] = None
    offset_inputs: bool = False
    side_stream: bool = False
    big: bool = False
    wpad: int = 0                                   # weight_stride - Nc
    rpad: int = 0                                   # row stride - width of every per-row table
    shared: bool = False                            # per-row tables: row 0's, once, with stride 0
    rows: Optional[Tuple[int, int]] = None
    cells: Optional[Tuple[int, int]] = None
    big_weights: bool = False


compact = Layout("compact")
offset_inputs = Layout("offset_inputs", offset_inputs=True)
side_stream = Layout("side_stream", side_stream=True)
big_stride = Layout("big_stride", big=True)
shared_tables = Layout("shared_tables", shared=True)
big_weight_stride = Layout("big_weight_stride", big_weights=True)


def padded(p):
    return Layout(f"padded({p})", pad=p)


def window(left, right):
    return Layout(f"window({left},{right})", left=left, right=right)


def gene_range(g0, g1):
    return Layout(f"gene_range({g0},{g1})", pad=3, genes=(g0, g1))


def weights_padded(p):
    return Layout(f"weights_padded({p})", wpad=p)


def row_strides(p):
    return Layout(f"row_strides({p})", rpad=p)


def row_range(b0, b1):
    return Layout(f"row_range({b0},{b1})", rows=(b0, b1))


def cell_range(c0, c1):
    return Layout(f"cell_range({c0},{c1})", cells=(c0, c1))


def both(a, b):
    """The layout with what a and b each change (no field changed by both)."""
    fields = {k: v for k, v in b.__dict__.items() if k != "name" and v != getattr(compact, k)}
    assert all(getattr(a, k) == getattr(compact, k) for k in fields)
    return replace(a, name=f"{a.name}+{b.name}", **fields)


# ------------------------------------------------------------------------------------------------------------ host buffers (numpy only)
def poison(dtype):
    return np.uint16(POISON_U16) if np.dtype(dtype) == np.uint16 else np.float32(np.nan)


def is_poison(x):
    return x == POISON_U16 if x.dtype == np.uint16 else np.isnan(x)


def other_counts(M, n, seed=OTHER_SEED):
    """[Ng][n] plausible counts of another seed at every gene's own level, in M's dtype."""
    rng = np.random.default_rng(seed)
    return rng.poisson(M.astype(np.float64).mean(1, keepdims=True) + 1.0, (M.shape[0], n)).astype(M.dtype)


def count_buffer(M, layout, second=False):
    """M [Ng][Nc] uint16 | float32 (the whole problem) -> (buf, base, gene_stride, Ng): the call reads element (g, c), g < Ng, at
    buf[base + g * gene_stride + c].  A window's buffer ends with `left` more poison elements, so that even a row walked to gene_stride
    from counts_dev stays inside it.  An odd padding is there to put uint16 rows on odd elements (addresses that are only 2-byte
    aligned): where Nc + p is odd every second row is; where it is even (Nc odd, as in most cases here) the block itself starts at
    element 1 of its allocation, so every row is.  second: the joint kernels' other layer, built in the same layout (one gene_stride
    holds for both) with the other lead wherever the block is not the compact one, so that row g of it stands on an odd element where
    row g of the first layer stands on an even one, and a window's left columns hold a third seed's counts.  A cell range is the
    compact block with counts_dev advanced by its first cell (real cells either side) and that many poison elements behind it."""
    assert not layout.big
    Ng, Nc = M.shape
    fill = lambda n: np.full(n, poison(M.dtype), dtype=M.dtype)                     # noqa: E731
    if layout.cells is not None:
        assert not (layout.pad or layout.left or layout.right or layout.genes)
        return np.concatenate([M.reshape(-1), fill(layout.cells[0])]), layout.cells[0], Nc, Ng
    width = layout.left + Nc + layout.pad + layout.right
    blk = np.full((Ng, width), poison(M.dtype), dtype=M.dtype)
    if layout.left:
        blk[:, :layout.left] = other_counts(M, layout.left, THIRD_SEED if second else OTHER_SEED)
    blk[:, layout.left:layout.left + Nc] = M
    lead = 1 if layout.pad % 2 == 1 and width % 2 == 0 else 0
    if second and width != Nc:
        lead = 1 - lead
    buf = np.concatenate([fill(lead), blk.reshape(-1), fill(layout.left)])
    g0, g1 = layout.genes if layout.genes is not None else (0, Ng)
    return buf, lead + layout.left + g0 * width, width, g1 - g0


def guarded(n, dtype, tail=0):
    """GUARD + n + GUARD + tail elements, every byte SENTINEL: an output of n elements with its two bands (tail: a longer band behind)."""
    return np.full((2 * GUARD + n + tail) * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype)


def bands_intact(whole, n=None):
    """Both bands of an output of n elements (None: all but 2 GUARD) still hold the sentinel in every byte."""
    b = whole.view(np.uint8)
    lo = GUARD * whole.dtype.itemsize
    hi = b.size - lo if n is None else (GUARD + n) * whole.dtype.itemsize
    return bool((b[:lo] == SENTINEL).all() and (b[hi:] == SENTINEL).all())


def row_output_block(R, n, Ng_all, width, dtype):
    """The guarded block [R][n][width] of a gene range's per-row outputs (n of Ng_all genes) -> (whole, elements of the body).  The band
    behind it is long enough to hold row R - 1 of an output laid out with the whole problem's Ng_all instead of the call's n."""
    return guarded(R * n * width, dtype, tail=R * (Ng_all - n) * width), R * n * width


def untouched(x):
    return bool((np.ascontiguousarray(x).view(np.uint8) == SENTINEL).all())


def big_row_start(g, second=False):
    """Element of the big allocation at which row g of the call starts (second: of the joint kernels' U layer)."""
    return BIG_BASE + g * BIG_STRIDE + (BIG_U_OFFSET if second else 0)


def bigw_row_start(b):
    """float32 element of the big weight allocation at which row b of the weights starts."""
    return BIG_BASE + b * BIG_STRIDE


def weight_buffer(Wt, layout):
    """Wt float32 [R_all][Nc] (the whole table) -> (buf, base, weight_stride, R): the call reads w_bc, b < R, at
    buf[base + b * weight_stride + c]; what lies between Nc and the stride is NaN."""
    assert not layout.big_weights
    R_all, Nc = Wt.shape
    stride = Nc + layout.wpad
    blk = np.full((R_all, stride), np.nan, dtype=np.float32)
    blk[:, :Nc] = Wt
    b0, b1 = layout.rows if layout.rows is not None else (0, R_all)
    return blk.reshape(-1), b0 * stride, stride, b1 - b0


def row_table_buffer(T, layout, per_gene=0):
    """T float64 [width] (one table shared by the rows) or [R_all][width] (one per row) -> (buf, base, row_stride): the call reads entry
    i of row b's table at buf[base + b * row_stride + i].  A shared table has stride 0; per-row tables stand width + rpad apart with NaN
    between them, or (layout.shared) only row 0's is there, with stride 0.  per_gene: numbers per gene of a per-gene table (nu: K,
    start: 2 or K + 2), whose view at the first gene of a gene range keeps the whole table's row stride."""
    g0 = layout.genes[0] if layout.genes is not None else 0
    if T.ndim == 1:
        return T.copy(), g0 * per_gene, 0
    R_all, width = T.shape
    if layout.shared:
        assert layout.rows is None and all(T[b].tobytes() == T[0].tobytes() for b in range(R_all))
        return np.concatenate([T[0], np.full((R_all - 1) * width, np.nan)]), g0 * per_gene, 0      # a stride of `width` finds NaN, inside
    stride = width + layout.rpad
    blk = np.full((R_all, stride), np.nan, dtype=T.dtype)
    blk[:, :width] = T
    b0 = layout.rows[0] if layout.rows is not None else 0
    return blk.reshape(-1), b0 * stride + g0 * per_gene, stride


# --------------------------------------------------------------------------------------------------------------------------- specs
def _matrix(kblk):
    """The block the kernels read, as numpy: uint16 (from its int16 bits) or float32."""
    a = kblk.contiguous().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _kind(M):
    return _lib.VC_COUNTS_U16 if M.dtype == np.uint16 else _lib.VC_COUNTS_F32


def _head(basis32, K, logm32):
    return [("counts",), ("kind",), ("Ng",), ("Nc",), ("stride",), ("cell", basis32), ("val", int(K)), ("cell", logm32)]


def _f32(t):
    return t.to(torch.float32).contiguous() if t is not None else None


def glm_spec(p, storage, null=False):
    """vc_gene_glm on a problem of tests/gene_glm_checker.py; null: the constant alone (K = 1 on the same tables), the worker's second call."""
    prior = p["prior"] if p["prior"] is not None else (None, None)
    counts = p["S"].astype(np.float32)
    basis, logm, r, pm, pp = GH.check_arguments(counts, G.directions(p["phis"]), p["n"], p["H"], p["a"], p["noisemodel"],
                                                p["dispersion"] if p["dispersion"] is not None else 0.3, prior[0], prior[1], TOL, MAX_ITER)
    blk, kblk, _ = GH._stage(counts, 0, counts.shape[1], counts.shape[0], CPU, storage)
    K = 1 if null else basis.shape[0]
    if null and pm is not None:
        pm, pp = pm[:, :1].contiguous(), pp[:, :1].contiguous()
    f8, i4 = np.float64, np.int32
    args = _head(_f32(basis), K, _f32(logm)) + [
        ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)), ("gene", pm), ("gene", pp), ("val", TOL), ("val", MAX_ITER),
        ("out", "nu", f8, (K,)), ("out", "cov", f8, (K * (K + 1) // 2,)), ("out", "ll", f8, ()), ("out", "dec", f8, ()),
        ("out", "it", i4, ()), ("out", "st", i4, ()), ("stream",)]
    return dict(fn="vc_gene_glm", M=_matrix(kblk), blk32=blk, r32=_f32(r), K=K, args=args)


def batch_spec(p, storage, null=False):
    """vc_gene_glm_batch on a problem of tests/gene_batch_checker.py, the cells sorted by batch as the worker sorts them."""
    prior = p["prior"] if p["prior"] is not None else (None, None)
    counts = p["S"].astype(np.float32)
    Nc, Ng = counts.shape
    basis, logm, r, pm, pp = GH.check_arguments(counts, G.directions(p["phis"]), p["n"], p["H"], p["a"], p["noisemodel"],
                                                p["dispersion"] if p["dispersion"] is not None else 0.3, prior[0], prior[1], TOL, MAX_ITER)
    labels, Nb = GB.batch_labels(p["labels"], Nc)
    dm, dq = GB.delta_prior(p["dprior"], Nb, Ng)
    perm, seg = GB.batch_segments(labels, Nb)
    blk, kblk, _ = GH._stage(counts, 0, Ng, Nc, CPU, storage)
    blk, kblk = blk[:, perm].contiguous(), kblk[:, perm].contiguous()
    K = 1 if null else basis.shape[0]
    if null and pm is not None:
        pm, pp = pm[:, :1].contiguous(), pp[:, :1].contiguous()
    f8, i4 = np.float64, np.int32
    args = _head(_f32(basis[:, perm]), K, _f32(logm[perm])) + [
        ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)), ("val", Nb), ("val", (C.c_int64 * (Nb + 1))(*seg)), ("gene", dm),
        ("gene", dq), ("gene", pm), ("gene", pp), ("val", TOL), ("val", MAX_ITER),
        ("out", "nu", f8, (K,)), ("out", "delta", f8, (Nb,)), ("out", "cov", f8, (K * (K + 1) // 2,)), ("out", "dvar", f8, (Nb,)),
        ("out", "ll", f8, ()), ("out", "dec", f8, ()), ("out", "it", i4, ()), ("out", "st", i4, ()), ("stream",)]
    return dict(fn="vc_gene_glm_batch", M=_matrix(kblk), blk32=blk, r32=_f32(r), K=K, Nb=Nb, args=args)


def dispersion_spec(p, storage, start=None, evaluate_only=False):
    """vc_gene_dispersion on a problem of tests/gene_dispersion_checker.py; start: a dispersion, as `gene_dispersion` takes it."""
    counts = p["S"].astype(np.float32)
    Nc, Ng = counts.shape
    basis, logm, r, _, _ = GH.check_arguments(counts, G.directions(p["phis"]), p["n"], p["H"], 1, "NegativeBinomial",
                                              0.3 if start is None else start, None, None, TOL, GH.DISPERSION_MAX_ITER)
    pa, pb = GH._dispersion_prior(p["prior"], Ng)
    blk, kblk, _ = GH._stage(counts, 0, Ng, Nc, CPU, storage)
    K = basis.shape[0]
    nu = torch.as_tensor(np.ascontiguousarray(np.asarray(p["nu"], dtype=np.float64).reshape(Ng, K)))
    f8, i4 = np.float64, np.int32
    args = _head(_f32(basis), K, _f32(logm)) + [
        ("gene", nu), ("gene", _f32(r) if start is not None else None), ("gene", pa), ("gene", pb), ("val", TOL),
        ("val", 0 if evaluate_only else GH.DISPERSION_MAX_ITER),
        ("out", "rho", f8, ()), ("out", "r", np.float32, ()), ("out", "info", f8, ()), ("out", "ll", f8, ()), ("out", "score", f8, ()),
        ("out", "it", i4, ()), ("out", "st", i4, ()), ("stream",)]
    return dict(fn="vc_gene_dispersion", M=_matrix(kblk), blk32=blk, K=K, args=args)


def kinetics_spec(p, storage):
    """vc_gene_kinetics on a problem of tests/gene_kinetics_checker.py, at its own coefficients of the angular speed on its own design."""
    from tests import gene_kinetics_checker as Q
    counts = p["U"].astype(np.float32)
    Nc, Ng = counts.shape
    dirs = Q.directions(p["phis"])
    basis, logm, nu, r, pr, st = GK.check_arguments(counts, dirs, p["n"], p["nu"].T, 1, p["noisemodel"],
                                                    1.0 / p["r"] if p["r"] is not None else 0.3, GK.DEFAULT_PRIOR, None, False, TOL, MAX_ITER)
    W = _f32(torch.as_tensor(GK.omega_design(dirs, p["Hw"], p["D"])))
    nuw = torch.as_tensor(np.ascontiguousarray(p["nuw"], dtype=np.float64))
    NW = int(W.shape[0])
    blk, kblk, _ = GH._stage(counts, 0, Ng, Nc, CPU, storage)
    f8, i4 = np.float64, np.int32
    args = _head(_f32(basis), basis.shape[0], _f32(logm)) + [
        ("gene", torch.as_tensor(nu)), ("cell", W), ("val", NW), ("plain", nuw), ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)),
        ("gene", torch.as_tensor(pr)), ("gene", None), ("val", TOL), ("val", MAX_ITER),
        ("out", "xy", f8, (2,)), ("out", "cov", f8, (3,)), ("out", "ll", f8, ()), ("out", "dec", f8, ()), ("out", "it", i4, ()),
        ("out", "st", i4, ()), ("out", "nc", i4, ()), ("out", "score", f8, (NW,)), ("out", "info", f8, (NW * (NW + 1) // 2,)), ("stream",)]
    return dict(fn="vc_gene_kinetics", M=_matrix(kblk), blk32=blk, r32=_f32(r), K=int(basis.shape[0]), NW=NW, args=args)


def mle_spec(S, T, n, noisemodel, dispersion, storage):
    """vc_phase_mle with the profile on (S [Nc, Ng], T [bins, Ng], n [Nc]) as `phase_mle` takes them."""
    Nc, Ng = S.shape
    T64, m64, r64 = PM.check_arguments(Nc, Ng, T, n, noisemodel, dispersion)
    T32, E32, m32, r32 = PM.stage_tables(T64, m64, r64)
    blk = PM._dense_block(S, 0, Nc, Ng, CPU)
    kblk = PM.u16_bits(blk) if storage == "u16" else blk
    bins = int(T32.shape[0])
    args = [("counts",), ("kind",), ("Ng",), ("Nc",), ("stride",), ("cell", T32.contiguous()), ("cell", E32.contiguous()), ("val", bins),
            ("cell", m32.contiguous()), ("val", _lib.NOISE[noisemodel]), ("plain", r32), ("cellout", "best_bin", np.int32, (Nc,)),
            ("cellout", "logp_rel", np.float32, (bins, Nc)), ("stream",)]
    return dict(fn="vc_phase_mle", M=_matrix(kblk), args=args)


def case_weights(Wt, rows=3):
    """The first `rows` rows of a bootstrap checker's table, float64 [rows][Nc], with a non-integer weight planted into row 1 -- the
    row that then holds, as every weighted case here must, both a cell of weight 0 and a weight that is no integer."""
    w = np.array(np.asarray(Wt)[:rows], dtype=np.float64)
    assert w.shape[0] == rows and (w[1] == 0).any()
    w[1, int(np.flatnonzero(w[1] > 0)[0])] += 0.75
    assert (w[1] == 0).any() and (w[1] != np.round(w[1])).any()
    return w


def _table32(Wt, Nc):
    """The float32 table the kernels read: the workers' `check_weights`, which a planted NaN (row isolation) has to go round."""
    w = np.asarray(Wt, dtype=np.float64)
    return GH.check_weights(w, Nc) if np.isfinite(w).all() else np.ascontiguousarray(w, dtype=np.float32)


def _pattern(*shape):
    """A fixed table of numbers in [-1, 1], different in every entry: what makes one row's (one gene's) table unlike the next."""
    return np.cos(1.0 + 0.7 * np.arange(int(np.prod(shape)), dtype=np.float64)).reshape(shape)


def _per_row(shared, R, scale, mode):
    """shared float64 [...] -> the per-row form of a table: "shared": itself (stride 0); "rows": [R][width], row b moved by
    scale (b + 1) x a fixed pattern; "copies": [R][width], R copies of "rows"' row 0."""
    if shared is None or mode == "shared":
        return None if shared is None else np.ascontiguousarray(shared, dtype=np.float64).reshape(-1)
    flat = np.asarray(shared, dtype=np.float64).reshape(-1)
    rows = np.stack([flat + scale * (b + 1) * _pattern(flat.size) for b in range(R)])
    return np.ascontiguousarray(rows if mode == "rows" else np.repeat(rows[:1], R, axis=0))


def _rouf(name, dtype, trail, wanted=True):
    return ("rout", name, dtype, trail) if wanted else ("val", None)


def glm_weighted_spec(p, Wt, storage, warm=False, want_cov=True):
    """vc_gene_glm_weighted on a problem of tests/gene_glm_checker.py under the rows Wt [R][Nc]; warm: a start per gene, near the
    default one and different for every gene (the bootstrap hands over the full-data fit)."""
    s = glm_spec(p, storage)
    Ng, Nc = s["M"].shape
    K = s["K"]
    start = None
    if warm:
        S = p["S"].astype(np.float64)
        start = np.zeros((Ng, K))
        start[:, 0] = np.log(np.maximum(S.sum(0), 0.5) / (np.asarray(p["n"], dtype=np.float64) ** p["a"]).sum())
        start = torch.from_numpy(np.clip(start + 0.01 * _pattern(Ng, K), -40.0, 40.0))
    f8, i4 = np.float64, np.int32
    head = s["args"][:12]                                           # counts .. prior_prec_dev, as vc_gene_glm takes them
    args = head + [("weights", _table32(Wt, Nc)), ("R",), ("wstride",), ("gene", start), ("val", TOL), ("val", MAX_ITER),
                   ("rout", "nu", f8, (K,)), _rouf("cov", f8, (K * (K + 1) // 2,), want_cov), ("rout", "ll", f8, ()), ("rout", "dec", f8, ()),
                   ("rout", "it", i4, ()), ("rout", "st", i4, ()), ("stream",)]
    return dict(s, fn="vc_gene_glm_weighted", args=args)


def batch_weighted_spec(p, Wt, storage, warm=False, want_var=True):
    """vc_gene_glm_batch_weighted on a problem of tests/gene_batch_checker.py; Wt [R][Nc] in the caller's cell order, permuted with the
    cells as the worker permutes it."""
    s = batch_spec(p, storage)
    Ng, Nc = s["M"].shape
    K, Nb = s["K"], s["Nb"]
    labels, _ = GB.batch_labels(p["labels"], Nc)
    perm, _ = GB.batch_segments(labels, Nb)
    start_nu = start_delta = None
    if warm:
        S = p["S"].astype(np.float64)
        nu = np.zeros((Ng, K))
        nu[:, 0] = np.log(np.maximum(S.sum(0), 0.5) / np.asarray(p["n"], dtype=np.float64).sum())
        start_nu = torch.from_numpy(np.clip(nu + 0.01 * _pattern(Ng, K), -40.0, 40.0))
        start_delta = torch.from_numpy(0.01 * _pattern(Ng, Nb))
    f8, i4 = np.float64, np.int32
    head = s["args"][:16]                                           # counts .. prior_prec_dev, as vc_gene_glm_batch takes them
    args = head + [("weights", np.ascontiguousarray(_table32(Wt, Nc)[:, perm])), ("R",), ("wstride",), ("gene", start_nu),
                   ("gene", start_delta), ("val", TOL), ("val", MAX_ITER), ("rout", "nu", f8, (K,)), ("rout", "delta", f8, (Nb,)),
                   _rouf("cov", f8, (K * (K + 1) // 2,), want_var), _rouf("dvar", f8, (Nb,), want_var), ("rout", "ll", f8, ()),
                   ("rout", "dec", f8, ()), ("rout", "it", i4, ()), ("rout", "st", i4, ()), ("stream",)]
    return dict(s, fn="vc_gene_glm_batch_weighted", args=args)


def _kinetics_staged(p, storage, nw0):
    from tests import gene_kinetics_checker as Q
    counts = p["U"].astype(np.float32)
    Nc, Ng = counts.shape
    dirs = Q.directions(p["phis"])
    basis, logm, nu, r, pr, _ = GK.check_arguments(counts, dirs, p["n"], p["nu"].T, 1, p["noisemodel"],
                                                   1.0 / p["r"] if p["r"] is not None else 0.3, GK.DEFAULT_PRIOR, None, False, TOL, MAX_ITER)
    W = None if nw0 else _f32(torch.as_tensor(GK.omega_design(dirs, p["Hw"], p["D"])))
    nuw = None if nw0 else np.ascontiguousarray(p["nuw"], dtype=np.float64)
    blk, kblk, _ = GH._stage(counts, 0, Ng, Nc, CPU, storage)
    return basis, logm, nu, r, pr, W, nuw, blk, kblk


def kinetics_weighted_spec(p, Wt, storage, tables="shared", want_cov=True, nw0=False):
    """vc_gene_kinetics_weighted on a problem of tests/gene_kinetics_checker.py under the rows Wt [R][Nc].  tables: "shared": the
    problem's own nu and nuw with strides 0 and no start (what the worker hands over for `cell_weights`); "rows": nu, nuw and a start
    per row, every row's different; "copies": R copies of "rows"' row 0 (what `shared_tables` is held to).  nw0: NW = 0."""
    basis, logm, nu, r, pr, W, nuw, blk, kblk = _kinetics_staged(p, storage, nw0)
    Ng, K = nu.shape
    R, NW = np.asarray(Wt).shape[0], 0 if nw0 else int(W.shape[0])
    nu_t = _per_row(nu, R, 0.01, tables)
    nuw_t = _per_row(nuw, R, 0.003, tables)
    start_t = None if tables == "shared" else _per_row(np.stack([p["x"], p["y"]], 1), R, 0.05, tables)
    f8, i4 = np.float64, np.int32
    args = _head(_f32(basis), K, _f32(logm)) + [
        ("rowtab", nu_t, K), ("cell", W), ("val", NW), ("rowtab", nuw_t, 0), ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)),
        ("gene", torch.as_tensor(pr)), ("weights", _table32(Wt, blk.shape[1])), ("R",), ("wstride",), ("rowtab", start_t, 2), ("val", TOL),
        ("val", MAX_ITER), ("rout", "xy", f8, (2,)), _rouf("cov", f8, (3,), want_cov), ("rout", "ll", f8, ()), ("rout", "dec", f8, ()),
        ("rout", "it", i4, ()), ("rout", "st", i4, ()), ("rout", "nc", i4, ()), ("rout", "score", f8, (NW,)),
        ("rout", "info", f8, (NW * (NW + 1) // 2,)), ("stream",)]
    return dict(fn="vc_gene_kinetics_weighted", M=_matrix(kblk), blk32=blk, r32=_f32(r), K=int(K), NW=NW, args=args)


def cell_speed_spec(p, storage, varied=False, max_iter=MAX_ITER):
    """vc_cell_speed on a problem of tests/cell_speed_checker.py from the checker's start without a prior (the worker's defaults);
    varied: a start and a Normal prior per cell, every cell's different, so that a cell read at the wrong index shows."""
    from tests import cell_speed_checker as Q
    from tests.gene_kinetics_checker import directions
    counts = p["U"].astype(np.float32)
    Nc, Ng = counts.shape
    keep, basis, logm, nu, xy, r = CSP.check_arguments(counts, directions(p["phis"]), p["n"], p["nu"].T, p["x"], p["y"], 1, p["noisemodel"],
                                                       1.0 / p["r"] if p["r"] is not None else 0.3, None, TOL, MAX_ITER)
    assert keep is None
    blk = PM._dense_block(counts, 0, Nc, Ng, CPU)
    kblk = PM.u16_bits(blk) if storage == "u16" else blk
    start = torch.from_numpy(np.full(Nc, Q.START) + (0.05 * _pattern(Nc) if varied else 0.0))
    pr = torch.from_numpy(np.stack([0.1 * _pattern(Nc), 3.0 + _pattern(Nc)], 1)) if varied else None
    K = int(basis.shape[0])
    f8, i4 = np.float64, np.int32
    args = [("counts",), ("kind",), ("Ng",), ("Nc",), ("stride",), ("basis", _f32(basis)), ("val", K), ("percell", _f32(logm)),
            ("gene", torch.as_tensor(nu)), ("gene", torch.as_tensor(xy)), ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)),
            ("percell", pr), ("percell", start), ("val", TOL), ("val", max_iter), ("cout", "omega", f8, ()), ("cout", "var", f8, ()),
            ("cout", "sums", f8, (6,)), ("cout", "dec", f8, ()), ("cout", "it", i4, ()), ("cout", "st", i4, ()), ("cout", "nc", i4, ()),
            ("stream",)]
    return dict(fn="vc_cell_speed", M=_matrix(kblk), blk32=blk, r32=_f32(r), K=K, args=args)


def _joint_staged(p, storage, nw0):
    from tests import gene_joint_checker as Q
    S, U = p["S"].astype(np.float32), p["U"].astype(np.float32)
    Nc, Ng = S.shape
    dirs = Q.directions(p["phis"])
    basis, logm, r, pm, pp, pr, _ = GJ.check_arguments(S, U, dirs, p["n"], p["H"], 1, p["noisemodel"],
                                                       1.0 / p["r"] if p["r"] is not None else 0.3, tol=TOL, max_iter=JOINT_MAX_ITER)
    W = None if nw0 else _f32(torch.as_tensor(GK.omega_design(dirs, p["Hw"], p["D"])))
    nuw = None if nw0 else np.ascontiguousarray(p["nuw"], dtype=np.float64)
    blkS, kS, kindS = GH._stage(S, 0, Ng, Nc, CPU, storage)
    blkU, kU, kindU = GH._stage(U, 0, Ng, Nc, CPU, storage)
    assert kindS == kindU
    return basis, logm, r, pm, pp, pr, W, nuw, blkS, kS, blkU, kU


def _joint_head(basis, K, logm):
    return [("counts",), ("counts2",), ("kind",), ("Ng",), ("Nc",), ("stride",), ("cell", basis), ("val", int(K)), ("cell", logm)]


def _joint_start(p):
    """[Ng][K + 2]: the simulation's truth, a finite point inside the box."""
    return np.concatenate([p["nu"], np.asarray(p["x"])[:, None], np.asarray(p["y"])[:, None]], 1)


def joint_spec(p, storage, nw0=False, start=False):
    """vc_gene_joint on a problem of tests/gene_joint_checker.py at its own coefficients of the angular speed on its own design."""
    basis, logm, r, pm, pp, pr, W, nuw, blkS, kS, blkU, kU = _joint_staged(p, storage, nw0)
    K, NW = int(basis.shape[0]), 0 if nw0 else int(W.shape[0])
    D = K + 2
    st = torch.from_numpy(_joint_start(p) + 0.02 * _pattern(blkS.shape[0], D)) if start else None
    f8, i4 = np.float64, np.int32
    args = _joint_head(_f32(basis), K, _f32(logm)) + [
        ("cell", W), ("val", NW), ("plain", nuw), ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)), ("gene", torch.as_tensor(pm)),
        ("gene", torch.as_tensor(pp)), ("gene", torch.as_tensor(pr)), ("gene", st), ("val", TOL), ("val", JOINT_MAX_ITER),
        ("out", "theta", f8, (D,)), ("out", "cov", f8, (D * (D + 1) // 2,)), ("out", "lls", f8, ()), ("out", "llu", f8, ()),
        ("out", "dec", f8, ()), ("out", "it", i4, ()), ("out", "st", i4, ()), ("out", "nc", i4, ()), ("out", "score", f8, (NW,)),
        ("out", "info", f8, (NW * (NW + 1) // 2,)), ("stream",)]
    return dict(fn="vc_gene_joint", M=_matrix(kS), M2=_matrix(kU), blk32=blkS, blk32_2=blkU, r32=_f32(r), K=K, NW=NW, args=args)


def joint_weighted_spec(p, Wt, storage, tables="shared", want_cov=True, nw0=False, start=None):
    """vc_gene_joint_weighted on a problem of tests/gene_joint_checker.py under the rows Wt [R][Nc]; tables as `kinetics_weighted_spec`
    takes them, over nuw and the start [Ng][K + 2].  start: with "shared" tables, one start [Ng][K + 2] for all rows (the bootstrap's
    warm start)."""
    basis, logm, r, pm, pp, pr, W, nuw, blkS, kS, blkU, kU = _joint_staged(p, storage, nw0)
    K, NW = int(basis.shape[0]), 0 if nw0 else int(W.shape[0])
    D, R = K + 2, np.asarray(Wt).shape[0]
    nuw_t = _per_row(nuw, R, 0.003, tables)
    start_t = _per_row(start, R, 0.0, "shared") if tables == "shared" else _per_row(_joint_start(p), R, 0.02, tables)
    f8, i4 = np.float64, np.int32
    args = _joint_head(_f32(basis), K, _f32(logm)) + [
        ("cell", W), ("val", NW), ("rowtab", nuw_t, 0), ("val", _lib.NOISE[p["noisemodel"]]), ("gene", _f32(r)), ("gene", torch.as_tensor(pm)),
        ("gene", torch.as_tensor(pp)), ("gene", torch.as_tensor(pr)), ("weights", _table32(Wt, blkS.shape[1])), ("R",), ("wstride",),
        ("rowtab", start_t, D), ("val", TOL), ("val", JOINT_MAX_ITER), ("rout", "theta", f8, (D,)),
        _rouf("cov", f8, (D * (D + 1) // 2,), want_cov), ("rout", "lls", f8, ()), ("rout", "llu", f8, ()), ("rout", "dec", f8, ()),
        ("rout", "it", i4, ()), ("rout", "st", i4, ()), ("rout", "nc", i4, ()), ("rout", "score", f8, (NW,)),
        ("rout", "info", f8, (NW * (NW + 1) // 2,)), ("stream",)]
    return dict(fn="vc_gene_joint_weighted", M=_matrix(kS), M2=_matrix(kU), blk32=blkS, blk32_2=blkU, r32=_f32(r), K=K, NW=NW, args=args)


def weights_of(spec):
    """The float32 table [R][Nc] of a weighted spec (None: the spec has none)."""
    for a in spec["args"]:
        if a[0] == "weights":
            return a[1]
    return None


def take_genes(spec, g0, g1):
    """The spec of genes [g0, g1) alone (per-gene kernels): the matrix rows, every per-gene input and every per-row per-gene table cut on
    the host."""
    assert spec["fn"] not in ("vc_phase_mle", "vc_cell_speed")
    Ng_all = spec["M"].shape[0]

    def cut(a):
        if a[0] == "gene":
            return ("gene", a[1][g0:g1].contiguous() if a[1] is not None else None)
        if a[0] == "rowtab" and a[1] is not None and a[2]:
            T = a[1].reshape(a[1].shape[:-1] + (Ng_all, a[2]))
            return ("rowtab", np.ascontiguousarray(T[..., g0:g1, :]).reshape(a[1].shape[:-1] + ((g1 - g0) * a[2],)), a[2])
        return a
    out = dict(spec, M=np.ascontiguousarray(spec["M"][g0:g1]), blk32=spec["blk32"][g0:g1].contiguous(), args=[cut(a) for a in spec["args"]])
    if "M2" in spec:
        out.update(M2=np.ascontiguousarray(spec["M2"][g0:g1]), blk32_2=spec["blk32_2"][g0:g1].contiguous())
    return out


# ----------------------------------------------------------------------------------------------------------------------- the call
_ballast = {}


def _ballast_pair(dev):
    if dev not in _ballast:
        _ballast[dev] = (torch.zeros(BALLAST_BYTES, dtype=torch.uint8, device=dev), torch.empty(BALLAST_BYTES, dtype=torch.uint8, device=dev))
    return _ballast[dev]


def _np(t):
    a = t.contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.int16) if a.dtype == np.uint16 else a


def big_allocation(dev):
    """The shared allocation of the 32-bit row-index tests: BIG_ALLOC uint16 elements, every byte 0xFF (one fill)."""
    return torch.empty(BIG_ALLOC, dtype=torch.int16, device=dev).fill_(-1)


def big_weight_allocation(dev):
    """The allocation of the 32-bit weight-row tests: BIGW_TOTAL float32 elements, every byte 0xFF (NaN; one fill)."""
    return torch.empty(BIGW_TOTAL, dtype=torch.int32, device=dev).fill_(-1)


def direct_call(spec, layout, dev=None, big=None):
    """ONE call of spec["fn"] in `layout`.  Returns name -> host array of every output (per-gene outputs: the rows of the call;
    per-row outputs [R][Ng][...]: the rows and genes of the call; per-cell outputs: the cells of the call), and "guards_intact" (both
    bands of every output, bit for bit), "outside_untouched" (the rows, genes or cells of the whole-problem outputs outside a range
    still hold the sentinel), "gene_stride", and for the weighted kernels "weight_stride" and "row_strides".  big: the tensor of
    `big_allocation` (layout big_stride) or of `big_weight_allocation` (layout big_weight_stride)."""
    lib = _lib.load()
    dev = torch.device(dev if dev is not None else f"cuda:{torch.cuda.current_device()}")
    M = spec["M"]
    Ng_all, Nc_all = M.shape
    g0, g1 = layout.genes if layout.genes is not None else (0, Ng_all)
    c0, c1 = layout.cells if layout.cells is not None else (0, Nc_all)
    Nc = c1 - c0
    Wt = weights_of(spec)
    R_all = Wt.shape[0] if Wt is not None else 1
    b0, b1 = layout.rows if layout.rows is not None else (0, R_all)
    assert 0 <= g0 < g1 <= Ng_all and 0 <= c0 < c1 <= Nc_all and 0 <= b0 < b1 <= R_all
    assert layout.cells is None or spec["fn"] == "vc_cell_speed"
    assert Wt is not None or not (layout.wpad or layout.rpad or layout.shared or layout.rows or layout.big_weights)
    assert layout.genes is None or layout.rows is None
    keep, pending, outs, row_strides = [], [], [], []
    with torch.cuda.device(dev):
        def upload(host):
            """A host array on the device; on a side stream a zeroed tensor that the stream fills behind its ballast copy."""
            src = torch.from_numpy(_np(host)).to(dev)
            if not layout.side_stream:
                keep.append(src)
                return src
            dst = torch.zeros_like(src)
            pending.append((dst, src))
            return dst

        M2, counts2_ptr = spec.get("M2"), None
        if layout.big:
            assert M.dtype == np.uint16 and M.shape == (BIG_NG, BIG_NC) and big is not None and big.numel() == BIG_ALLOC
            for g in range(BIG_NG):
                big[big_row_start(g):big_row_start(g) + Nc] = torch.from_numpy(_np(M[g])).to(dev)
            counts_ptr, stride, Ng = big.data_ptr() + 2 * BIG_BASE, BIG_STRIDE, BIG_NG
            if M2 is not None:
                assert M2.dtype == np.uint16 and M2.shape == M.shape
                for g in range(BIG_NG):
                    big[big_row_start(g, True):big_row_start(g, True) + Nc] = torch.from_numpy(_np(M2[g])).to(dev)
                counts2_ptr = counts_ptr + 2 * BIG_U_OFFSET
        else:
            buf, base, stride, Ng = count_buffer(M, layout)
            counts_ptr = upload(buf).data_ptr() + base * buf.dtype.itemsize
            if M2 is not None:
                buf2, base2, stride2, _ = count_buffer(M2, layout, second=True)
                assert stride2 == stride and M2.dtype == M.dtype and M2.shape == M.shape
                counts2_ptr = upload(buf2).data_ptr() + base2 * buf2.dtype.itemsize

        R, wstride, weights_ptr = b1 - b0, None, None
        if layout.big_weights:
            assert Wt.shape == (BIGW_ROWS, BIG_NC) and big is not None and big.numel() == BIGW_TOTAL and big.dtype == torch.int32
            for b in range(BIGW_ROWS):
                big[bigw_row_start(b):bigw_row_start(b) + Nc] = torch.from_numpy(Wt[b].view(np.int32).copy()).to(dev)
            weights_ptr, wstride = big.data_ptr() + 4 * BIG_BASE, BIG_STRIDE
        elif Wt is not None:
            wbuf, wbase, wstride, R = weight_buffer(Wt, layout)
            weights_ptr = upload(wbuf).data_ptr() + 4 * wbase

        def cell(t):
            if t is None:
                return None
            a = _np(t).reshape(-1)
            lead = ODD if layout.offset_inputs else 0
            host = a
            if lead:
                host = np.full(lead + a.size + lead + 1, np.nan, dtype=a.dtype)
                host[lead:lead + a.size] = a
            return upload(host).data_ptr() + lead * a.dtype.itemsize

        def gene(t):
            if t is None:
                return None
            a = _np(t)
            assert a.shape[0] == Ng_all
            return upload(a).data_ptr() + g0 * (a.size // Ng_all) * a.dtype.itemsize

        def out(name, dtype, trail, per_gene):
            width = int(np.prod(trail, dtype=np.int64))
            n = Ng_all * width if per_gene else width
            if n == 0:                                              # an output the call does not have (NW = 0)
                return None
            d = torch.from_numpy(guarded(n, dtype)).to(dev)
            outs.append((name, d, dtype, trail, "gene" if per_gene else "whole", n))
            return d.data_ptr() + (GUARD + (g0 * width if per_gene else 0)) * np.dtype(dtype).itemsize

        def percell(t):
            """A table with one entry per cell in front: the view at the first cell of a cell range, else a per-cell input like any."""
            if t is None or layout.cells is None:
                return cell(t)
            a = _np(t)
            assert a.shape[0] == Nc_all
            return upload(a).data_ptr() + c0 * (a.size // Nc_all) * a.dtype.itemsize

        def basis(t):
            """float[K][Nc]: the header fixes its row stride to Nc, so a cell range gets its own packed copy."""
            a = _np(t)
            assert a.shape[1] == Nc_all
            return cell(np.ascontiguousarray(a[:, c0:c1]))

        def rowtab(T, per_gene):
            if T is None:
                row_strides.append(0)
                return None, 0
            tbuf, tbase, tstride = row_table_buffer(T, layout, per_gene)
            row_strides.append(tstride)
            return upload(tbuf).data_ptr() + 8 * tbase, tstride

        def rout(name, dtype, trail):
            """[R][Ng][...]: of a gene range the call's own [R][g1 - g0] block, else the view at row b0 of the whole problem's."""
            width = int(np.prod(trail, dtype=np.int64))
            if width == 0:
                return None
            if layout.genes is not None:
                whole, n = row_output_block(R, g1 - g0, Ng_all, width, dtype)
                d, at = torch.from_numpy(whole).to(dev), 0
            else:
                n, at = R_all * Ng_all * width, b0 * Ng_all * width
                d = torch.from_numpy(guarded(n, dtype)).to(dev)
            outs.append((name, d, dtype, trail, "rows", n))
            return d.data_ptr() + (GUARD + at) * np.dtype(dtype).itemsize

        def cout(name, dtype, trail):
            width = int(np.prod(trail, dtype=np.int64))
            d = torch.from_numpy(guarded(Nc_all * width, dtype)).to(dev)
            outs.append((name, d, dtype, trail, "cells", Nc_all * width))
            return d.data_ptr() + (GUARD + c0 * width) * np.dtype(dtype).itemsize

        argv = []
        for a in spec["args"]:
            role = a[0]
            if role == "counts":
                argv.append(counts_ptr)
            elif role == "kind":
                argv.append(_kind(M))
            elif role == "Ng":
                argv.append(Ng)
            elif role == "Nc":
                argv.append(Nc)
            elif role == "stride":
                argv.append(stride)
            elif role == "val":
                argv.append(a[1])
            elif role == "cell":
                argv.append(cell(a[1]))
            elif role == "gene":
                argv.append(gene(a[1]))
            elif role == "plain":
                argv.append(upload(_np(a[1])).data_ptr() if a[1] is not None else None)
            elif role in ("out", "cellout"):
                argv.append(out(a[1], a[2], a[3], role == "out"))
            elif role == "counts2":
                argv.append(counts2_ptr)
            elif role == "weights":
                argv.append(weights_ptr)
            elif role == "R":
                argv.append(R)
            elif role == "wstride":
                argv.append(wstride)
            elif role == "rowtab":
                argv.extend(rowtab(a[1], a[2]))
            elif role == "rout":
                argv.append(rout(a[1], a[2], a[3]))
            elif role == "percell":
                argv.append(percell(a[1]))
            elif role == "basis":
                argv.append(basis(a[1]))
            elif role == "cout":
                argv.append(cout(a[1], a[2], a[3]))
            else:
                assert role == "stream"
                argv.append(None)
        torch.cuda.synchronize(dev)                                 # every allocation and fill is complete
        if layout.side_stream:
            stream = torch.cuda.Stream(dev)
            src, dst = _ballast_pair(dev)
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)
                for d, s in pending:
                    d.copy_(s, non_blocking=True)
        else:
            stream = torch.cuda.current_stream(dev)
        argv[-1] = C.c_void_p(stream.cuda_stream)
        rc = getattr(lib, spec["fn"])(*argv)
        stream.synchronize()
        if rc != _lib.VC_OK:
            raise RuntimeError(f"{spec['fn']} failed ({rc}): {lib.vc_last_error(None).decode()}")
        if layout.big and M2 is not None:                           # the other kernels' truncated indices must go on finding poison there
            for g in range(BIG_NG):
                big[big_row_start(g, True):big_row_start(g, True) + Nc].fill_(-1)
        res = dict(guards_intact=True, outside_untouched=True, gene_stride=stride)
        if Wt is not None:
            res.update(weight_stride=wstride, row_strides=tuple(row_strides))
        for name, d, dtype, trail, kind, n in outs:
            whole = d.cpu().numpy()
            res["guards_intact"] &= bands_intact(whole, n)
            body = whole[GUARD:GUARD + n]
            if kind == "gene":
                body = body.reshape((Ng_all,) + tuple(trail))
                res["outside_untouched"] &= untouched(body[:g0]) and untouched(body[g1:])
                res[name] = body[g0:g1].copy()
            elif kind == "rows" and layout.genes is not None:
                res[name] = body.reshape((R, g1 - g0) + tuple(trail)).copy()
            elif kind == "rows":
                body = body.reshape((R_all, Ng_all) + tuple(trail))
                res["outside_untouched"] &= untouched(body[:b0]) and untouched(body[b1:])
                res[name] = body[b0:b1].copy()
            elif kind == "cells":
                body = body.reshape((Nc_all,) + tuple(trail))
                res["outside_untouched"] &= untouched(body[:c0]) and untouched(body[c1:])
                res[name] = body[c0:c1].copy()
            else:
                res[name] = body.reshape(trail).copy()
        del keep, pending, outs
        return res


OUTPUT_FLAGS = ("guards_intact", "outside_untouched", "gene_stride", "weight_stride", "row_strides")


def assert_same_outputs(got, want):
    """Every output: same dtype and same bytes (NaN equal to NaN), and no NaN where `want` has none."""
    names = [k for k in want if k not in OUTPUT_FLAGS]
    assert sorted(names) == sorted(k for k in got if k not in OUTPUT_FLAGS)
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].dtype.kind == "f":
            assert not (np.isnan(got[k]) & ~np.isnan(want[k])).any(), k
        assert got[k].tobytes() == want[k].tobytes(), k
