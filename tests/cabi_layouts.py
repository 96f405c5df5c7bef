"""Direct calls of the five engine-less entry points of include/velocycle_hip.h -- vc_gene_glm, vc_gene_glm_batch, vc_gene_dispersion,
vc_gene_kinetics, vc_phase_mle -- in every memory layout the header allows, not only the one the Python workers use.

A *spec* is one problem staged on the host by the workers' own staging (`check_arguments`, `fourier_basis_from_directions`, `_stage`'s
uint16 bits, `gene_batch`'s sort and segments, `phase_mle.stage_tables`): the count matrix as the kernels read it, [genes][cells], and
the entry point's argument list with a role per argument.  A *layout* says where those arrays stand in device memory.  `direct_call`
makes ONE `lib.vc_*` call of a spec in a layout and returns every output as a host array, with the state of the guard bands around them.

Layouts (what each one catches):
  compact            gene_stride == Nc, fresh allocations: the workers' convention
  padded(p)          the count block is [Ng][Nc + p], the padding poison (0xFFFF | NaN): a row base formed with Nc, a row walked to
                     gene_stride; odd p puts uint16 rows on addresses that are only 2-byte aligned (`count_buffer`)
  window(l, r)       the block is [Ng][l + Nc + r], counts_dev advanced by l, gene_stride the full width: the zero-copy way to cut cells;
                     the left columns hold counts of another seed (a neighbour's cell gives another number, not a NaN), the right poison
  gene_range(a, b)   counts_dev at row a of the whole padded(3) block, every per-gene input and output the view at a of a whole-problem
                     tensor: the cut of the genes into calls; rows outside [a, b) of the outputs must keep their sentinel
  offset_inputs      every per-cell input is a view at an odd element of a larger NaN tensor: an alignment taken for granted
  side_stream        inputs produced and kernel launched on a fresh stream behind one large copy: a launch on another stream reads zeros
  big_stride         gene_stride = 2^30 + 1 with counts_dev 2^31 elements into an allocation filled with 0xFF: a row index formed in 32 bits
In every layout every output lives inside a larger tensor with GUARD elements of a fixed bit pattern before and after it.

Importing this module needs no GPU: the buffers are built with numpy (tests/test_cabi_layouts_cpu.py checks them there)."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from tests import gene_glm_checker as G
from velocycle_amd import _lib
from velocycle_amd import gene_batch as GB
from velocycle_amd import gene_harmonics as GH
from velocycle_amd import gene_kinetics as GK
from velocycle_amd import phase_mle as PM

GUARD = 64                       # elements of the sentinel before and after every output
SENTINEL = 0xA5                  # every byte of a guard band, and of an output before the launch
POISON_U16 = 0xFFFF
ODD = 3                          # the element an offset input starts at
OTHER_SEED = 77                  # of the counts in a window's left columns
BIG_STRIDE = (1 << 30) + 1
BIG_BASE = 1 << 31               # elements in front of counts_dev in the big allocation
BIG_NG, BIG_NC = 3, 257
BIG_TOTAL = BIG_BASE + (BIG_NG - 1) * BIG_STRIDE + BIG_NC          # uint16 elements: about 8.6 GB
BIG_FREE_NEEDED = 12 * 10 ** 9     # bytes that must be free for the 32-bit row-index tests to run
BALLAST_BYTES = 1 << 30          # the copy a side stream makes first: about a millisecond, a launch takes microseconds
CPU = torch.device("cpu")
TOL, MAX_ITER = 1e-10, 25        # the workers' defaults


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


compact = Layout("compact")
offset_inputs = Layout("offset_inputs", offset_inputs=True)
side_stream = Layout("side_stream", side_stream=True)
big_stride = Layout("big_stride", big=True)


def padded(p):
    return Layout(f"padded({p})", pad=p)


def window(left, right):
    return Layout(f"window({left},{right})", left=left, right=right)


def gene_range(g0, g1):
    return Layout(f"gene_range({g0},{g1})", pad=3, genes=(g0, g1))


# ------------------------------------------------------------------------------------------------------------ host buffers (numpy only)
def poison(dtype):
    return np.uint16(POISON_U16) if np.dtype(dtype) == np.uint16 else np.float32(np.nan)


def is_poison(x):
    return x == POISON_U16 if x.dtype == np.uint16 else np.isnan(x)


def other_counts(M, n):
    """[Ng][n] plausible counts of another seed at every gene's own level, in M's dtype."""
    rng = np.random.default_rng(OTHER_SEED)
    return rng.poisson(M.astype(np.float64).mean(1, keepdims=True) + 1.0, (M.shape[0], n)).astype(M.dtype)


def count_buffer(M, layout):
    """M [Ng][Nc] uint16 | float32 (the whole problem) -> (buf, base, gene_stride, Ng): the call reads element (g, c), g < Ng, at
    buf[base + g * gene_stride + c].  A window's buffer ends with `left` more poison elements, so that even a row walked to gene_stride
    from counts_dev stays inside it.  An odd padding is there to put uint16 rows on odd elements (addresses that are only 2-byte
    aligned): where Nc + p is odd every second row is; where it is even (Nc odd, as in most cases here) the block itself starts at
    element 1 of its allocation, so every row is."""
    assert not layout.big
    Ng, Nc = M.shape
    width = layout.left + Nc + layout.pad + layout.right
    blk = np.full((Ng, width), poison(M.dtype), dtype=M.dtype)
    if layout.left:
        blk[:, :layout.left] = other_counts(M, layout.left)
    blk[:, layout.left:layout.left + Nc] = M
    lead = 1 if layout.pad % 2 == 1 and width % 2 == 0 else 0
    fill = lambda n: np.full(n, poison(M.dtype), dtype=M.dtype)                     # noqa: E731
    buf = np.concatenate([fill(lead), blk.reshape(-1), fill(layout.left)])
    g0, g1 = layout.genes if layout.genes is not None else (0, Ng)
    return buf, lead + layout.left + g0 * width, width, g1 - g0


def guarded(n, dtype):
    """GUARD + n + GUARD elements, every byte SENTINEL: an output of n elements with its two bands."""
    return np.full((2 * GUARD + n) * np.dtype(dtype).itemsize, SENTINEL, dtype=np.uint8).view(dtype)


def bands_intact(whole):
    b = whole.view(np.uint8)
    n = GUARD * whole.dtype.itemsize
    return bool((b[:n] == SENTINEL).all() and (b[-n:] == SENTINEL).all())


def untouched(x):
    return bool((np.ascontiguousarray(x).view(np.uint8) == SENTINEL).all())


def big_row_start(g):
    """Element of the big allocation at which row g of the call starts."""
    return BIG_BASE + g * BIG_STRIDE


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


def take_genes(spec, g0, g1):
    """The spec of genes [g0, g1) alone (per-gene kernels): the matrix rows and every per-gene input cut on the host."""
    assert spec["fn"] != "vc_phase_mle"
    args = [("gene", a[1][g0:g1].contiguous() if a[1] is not None else None) if a[0] == "gene" else a for a in spec["args"]]
    return dict(spec, M=np.ascontiguousarray(spec["M"][g0:g1]), blk32=spec["blk32"][g0:g1].contiguous(), args=args)


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
    """The shared allocation of the 32-bit row-index tests: BIG_TOTAL uint16 elements, every byte 0xFF (one fill)."""
    return torch.empty(BIG_TOTAL, dtype=torch.int16, device=dev).fill_(-1)


def direct_call(spec, layout, dev=None, big=None):
    """ONE call of spec["fn"] in `layout`.  Returns name -> host array of every output (per-gene outputs: the rows of the call), and
    "guards_intact" (both bands of every output, bit for bit), "outside_untouched" (the rows of the whole-problem outputs outside a
    gene range still hold the sentinel), "gene_stride".  big: the tensor of `big_allocation` (layout big_stride)."""
    lib = _lib.load()
    dev = torch.device(dev if dev is not None else f"cuda:{torch.cuda.current_device()}")
    M = spec["M"]
    Ng_all, Nc = M.shape
    g0, g1 = layout.genes if layout.genes is not None else (0, Ng_all)
    keep, pending, outs = [], [], []
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

        if layout.big:
            assert M.dtype == np.uint16 and M.shape == (BIG_NG, BIG_NC) and big is not None and big.numel() == BIG_TOTAL
            for g in range(BIG_NG):
                big[big_row_start(g):big_row_start(g) + Nc] = torch.from_numpy(_np(M[g])).to(dev)
            counts_ptr, stride, Ng = big.data_ptr() + 2 * BIG_BASE, BIG_STRIDE, BIG_NG
        else:
            buf, base, stride, Ng = count_buffer(M, layout)
            counts_ptr = upload(buf).data_ptr() + base * buf.dtype.itemsize

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
            outs.append((name, d, dtype, trail, per_gene))
            return d.data_ptr() + (GUARD + (g0 * width if per_gene else 0)) * np.dtype(dtype).itemsize

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
        res = dict(guards_intact=True, outside_untouched=True, gene_stride=stride)
        for name, d, dtype, trail, per_gene in outs:
            whole = d.cpu().numpy()
            res["guards_intact"] &= bands_intact(whole)
            body = whole[GUARD:whole.size - GUARD]
            if per_gene:
                body = body.reshape((Ng_all,) + tuple(trail))
                res["outside_untouched"] &= untouched(body[:g0]) and untouched(body[g1:])
                res[name] = body[g0:g1].copy()
            else:
                res[name] = body.reshape(trail).copy()
        del keep, pending, outs
        return res


OUTPUT_FLAGS = ("guards_intact", "outside_untouched", "gene_stride")


def assert_same_outputs(got, want):
    """Every output: same dtype and same bytes (NaN equal to NaN), and no NaN where `want` has none."""
    names = [k for k in want if k not in OUTPUT_FLAGS]
    assert sorted(names) == sorted(k for k in got if k not in OUTPUT_FLAGS)
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].dtype.kind == "f":
            assert not (np.isnan(got[k]) & ~np.isnan(want[k])).any(), k
        assert got[k].tobytes() == want[k].tobytes(), k
