"""Maximum-likelihood phase assignment on a grid of bins (the worker behind `Phases.from_cycle_mle`; reference
velocycle/phases.py:471-509) on the HIP kernel `vc_phase_mle`.

For every cell c and bin j:  logP[j, c] = sum_g log p(k_gc | mu = exp(T[j, g]) * m_c),  Poisson or negative binomial
(`GammaPoisson(1 / dispersion, 1 / (dispersion * mu))`).  The kernel evaluates only what depends on the bin, keeps nothing of size
bins x genes x cells, and returns the best bin per cell (first of equal bins) and, on request, logP - max_j logP.

Cells are independent: they are walked in chunks, each chunk a dense [genes][cells] device block (a sparse layer is scattered into
it on the device -- the whole matrix is never densified on the host), and the result does not depend on the chunk size bit for bit.
There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_BINS = 4096                      # csrc/vc_phase_mle.hip
CHUNK_BYTES = 256 << 20              # bound of one chunk's dense float32 count block on the device
NOISEMODELS = ("Poisson", "NegativeBinomial")


def _is_sparse(x):
    return hasattr(x, "tocsr") and hasattr(x, "toarray")


def default_chunk_cells(Ng: int) -> int:
    """Cells per chunk such that the chunk's dense float32 block stays within CHUNK_BYTES (a multiple of 64, at least 64)."""
    return max(64, (CHUNK_BYTES // (4 * int(Ng))) // 64 * 64)


def check_arguments(Nc, Ng, T, m, noisemodel, dispersion):
    """Every refusal that needs no device.  Returns (T float64 [bins, Ng], m float64 [Nc], r float64 [Ng] or None)."""
    if noisemodel not in NOISEMODELS:
        raise NotImplementedError("Not implemented yet, sorry")
    T = torch.as_tensor(T).detach().to("cpu", torch.float64)
    if T.ndim != 2 or T.shape[0] < 1:
        raise ValueError("bins must be >= 1")
    if T.shape[0] > MAX_BINS:
        raise ValueError(f"bins must be <= {MAX_BINS}")
    if T.shape[1] != Ng or Ng < 1 or Nc < 1:
        raise ValueError(f"T has {T.shape[1]} genes, the counts have {Ng} (cells: {Nc})")
    if not bool(torch.isfinite(T).all()):
        raise ValueError("T must be finite")
    m = torch.as_tensor(m).detach().to("cpu", torch.float64).reshape(-1)
    if m.numel() != Nc:
        raise ValueError(f"m has {m.numel()} entries for {Nc} cells")
    if not bool((torch.isfinite(m) & (m > 0)).all()):
        raise ValueError("every cell needs a finite count factor > 0 (n_scounts <= 0?)")
    r = None
    if noisemodel == "NegativeBinomial":
        d = torch.as_tensor(np.asarray(dispersion, dtype=np.float64)).reshape(-1)
        if d.numel() not in (1, Ng):
            raise ValueError(f"dispersion must be a scalar or one value per gene ({Ng}), got {d.numel()}")
        if not bool((torch.isfinite(d) & (d > 0)).all()):
            raise ValueError("dispersion must be > 0")
        r = (1.0 / d).expand(Ng).contiguous()
    return T, m, r


def _dense_block(counts, c0, c1, Ng, dev):
    """Cells [c0, c1) as a float32 device block [Ng][c1 - c0], truncated to integers like `.astype(np.int64)`."""
    n = c1 - c0
    if _is_sparse(counts):
        sub = counts[c0:c1].tocoo()
        blk = torch.zeros((Ng, n), dtype=torch.float32, device=dev)
        if sub.nnz:
            rows = torch.from_numpy(sub.row.astype(np.int64)).to(dev)
            cols = torch.from_numpy(sub.col.astype(np.int64)).to(dev)
            val = torch.from_numpy(np.asarray(sub.data, dtype=np.float32)).to(dev)
            blk.index_put_((cols, rows), val, accumulate=True)
        return blk.trunc_()
    part = counts[c0:c1]
    part = part if torch.is_tensor(part) else torch.from_numpy(np.ascontiguousarray(part))
    return part.to(dev).to(torch.float32).T.clone(memory_format=torch.contiguous_format).trunc_()


def u16_bits(blk):
    """A float32 block of integers <= 65535 -> int16 holding the bits of the uint16 values (what VC_COUNTS_U16 reads)."""
    blk = blk.to(torch.int32)
    blk[blk >= 32768] -= 65536
    return blk.to(torch.int16)


def stage_tables(T, m, r):
    """The float32 tables the kernel reads, on the host, from what `check_arguments` returns: (T - s, exp(T - s), m e^s, r or None).
    mu = exp(T) m is unchanged by (T - s, m e^s): with s = mean(T) the kernel's tables are O(1) and its differences of logarithms
    cancel a few digits less.  s depends on the cycle only, so every cell is still assigned independently of the others."""
    s = T.mean()
    Tc = T - s
    return (Tc.to(torch.float32), torch.exp(Tc).to(torch.float32), (m * torch.exp(s)).to(torch.float32),
            r.to(torch.float32) if r is not None else None)


def phase_mle(counts, T, m, noisemodel="Poisson", dispersion=0.3, *, device=None, chunk_cells=None, return_profile=False,
              storage="auto"):
    """counts: [Nc, Ng] cell-major like an AnnData layer (numpy, scipy sparse or torch, host or device); T: [bins, Ng] log-rates per
    unit count factor (natural log; float64 keeps its digits through the centring below); m: [Nc] count factors (n_c^a);
    dispersion: scalar or [Ng].  storage: "auto" (uint16 per chunk when every count is an integer <= 65535) | "f32" | "u16".
    Returns (best_bin int64 [Nc], logp_rel float32 [bins, Nc] or None), both on the device."""
    Nc, Ng = int(counts.shape[0]), int(counts.shape[1])
    T, m, r = check_arguments(Nc, Ng, T, m, noisemodel, dispersion)
    if storage not in ("auto", "f32", "u16"):
        raise ValueError(f"unknown storage {storage!r}")
    if chunk_cells is not None and int(chunk_cells) < 1:
        raise ValueError("chunk_cells must be >= 1")
    lib = _lib.load()
    from .engine import HipEngineError
    if not torch.cuda.is_available():
        raise HipEngineError("velocycle_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    bins = T.shape[0]
    T32, E32, m32, r32 = stage_tables(T, m, r)
    with torch.cuda.device(dev):
        T_d = T32.to(dev).contiguous()
        E_d = E32.to(dev).contiguous()
        m_d = m32.to(dev).contiguous()
        r_d = r32.to(dev).contiguous() if r32 is not None else None
        best = torch.empty(Nc, dtype=torch.int32, device=dev)
        prof = torch.empty((bins, Nc), dtype=torch.float32, device=dev) if return_profile else None
        step = int(chunk_cells) if chunk_cells is not None else default_chunk_cells(Ng)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for c0 in range(0, Nc, step):
            c1 = min(Nc, c0 + step)
            n = c1 - c0
            blk = _dense_block(counts, c0, c1, Ng, dev)
            lo, hi = float(blk.min()), float(blk.max())
            if not (lo >= 0.0 and np.isfinite(hi)):
                raise ValueError("counts must be finite and >= 0")
            if storage == "u16" and hi > 65535:
                raise ValueError("storage='u16' needs every count <= 65535")
            if storage != "f32" and hi <= 65535:
                blk = u16_bits(blk)
                kind = _lib.VC_COUNTS_U16
            else:
                kind = _lib.VC_COUNTS_F32
            m_c = m_d[c0:c1]
            best_c = best[c0:c1]
            prof_c = torch.empty((bins, n), dtype=torch.float32, device=dev) if return_profile else None
            rc = lib.vc_phase_mle(C.c_void_p(blk.data_ptr()), kind, Ng, n, n, C.c_void_p(T_d.data_ptr()), C.c_void_p(E_d.data_ptr()),
                                  bins, C.c_void_p(m_c.data_ptr()), _lib.NOISE[noisemodel],
                                  C.c_void_p(r_d.data_ptr()) if r_d is not None else None, C.c_void_p(best_c.data_ptr()),
                                  C.c_void_p(prof_c.data_ptr()) if prof_c is not None else None, stream)
            if rc != _lib.VC_OK:
                raise HipEngineError(f"vc_phase_mle failed ({rc}): {lib.vc_last_error(None).decode()}")
            if prof_c is not None:
                prof[:, c0:c1] = prof_c
            del blk
        return best.to(torch.int64), prof
