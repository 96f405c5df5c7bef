"""Principal-component scores of the log counts on the device: the worker behind `Phases.from_pca_heuristic(device=...)`
(reference velocycle/phases.py:307-382, where it is np.log of a dense layer and sklearn's PCA on the host).

The first n <= 4 principal directions are found by a block power iteration with Rayleigh-Ritz extraction (block size 8).  Its only
large operation is one pass over the staged matrix per iteration, the HIP kernel `vc_pca_apply`:  Y = (X - mu) Q  and
Z = (X - mu)^T Y.  The loop around it (QR and the 8 x 8 eigenproblem, float64, through torch) is plumbing.

    stage     X = float32(log(float32(v) + float32(small_count))), resident on the device; float64 column sums (`vc_pca_stage`)
    start     Q = qr(standard-normal (Ng, 8) block from a CPU torch.Generator seeded with random_state, float64)
    iterate   (Y, Z) = apply(Q);  H = sym(Q^T Z);  theta, W = eigh(H) descending;  V = Q W
              residual = max_{j<n} ||Z W_j - theta_j V_j|| / theta_1;  stop at residual <= tol, else Q = qr(Z)
    finish    sign: the entry of largest magnitude of every component is positive (the first one on ties; sklearn's
              svd_flip(u_based_decision=False));  pcs = (X - mu) V[:, :n] from one more pass;  explained_variance_ = theta / (Nc - 1)

`device="cpu"` runs the same loop with float32 torch matmuls in place of the two kernels (so that a machine without a GPU exercises
everything but the kernels); a "cuda" device has no fallback: a missing library or kernel is an error.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

BLOCK = 8                            # csrc/vc_pca.hip: PCA_K
MAX_COMPONENTS = 4
CHUNK_BYTES = 256 << 20              # bound of one chunk's dense float32 block of raw values on the device


@dataclass
class PCAScores:
    """What `pca_scores` returns (and `Phases.from_pca_heuristic(device=...)` keeps as `.pca`)."""
    pcs: torch.Tensor                # (Nc, n) float32, on the device
    components_: np.ndarray          # (n, Ng) float64
    explained_variance_: np.ndarray  # (n,) float64
    mean_: np.ndarray                # (Ng,) float64
    n_iter_: int
    residual_: float
    converged_: bool


def _is_sparse(x):
    return hasattr(x, "tocsr") and hasattr(x, "toarray")


def default_chunk_cells(Ng: int) -> int:
    """Cells per chunk such that the chunk's dense float32 block stays within CHUNK_BYTES (a multiple of 64, at least 64)."""
    return max(64, (CHUNK_BYTES // (4 * int(Ng))) // 64 * 64)


def _free_bytes(dev: torch.device) -> int:
    if dev.type == "cuda":
        return int(torch.cuda.mem_get_info(dev)[0])
    return int(os.sysconf("SC_AVPHYS_PAGES")) * int(os.sysconf("SC_PAGE_SIZE"))


def _dense_block(layer, c0, c1, Ng, dev):
    """Cells [c0, c1) of the layer as a contiguous float32 block [c1 - c0][Ng] on `dev`."""
    if _is_sparse(layer):
        sub = layer[c0:c1].tocoo()
        blk = torch.zeros((c1 - c0, Ng), dtype=torch.float32, device=dev)
        if sub.nnz:
            rows = torch.from_numpy(sub.row.astype(np.int64)).to(dev)
            cols = torch.from_numpy(sub.col.astype(np.int64)).to(dev)
            val = torch.from_numpy(np.asarray(sub.data, dtype=np.float32)).to(dev)
            blk.index_put_((rows, cols), val, accumulate=True)
        return blk
    part = layer[c0:c1]
    if not torch.is_tensor(part):
        with warnings.catch_warnings():                      # a read-only array (a memory map, say) is only read here
            warnings.simplefilter("ignore", UserWarning)
            part = torch.from_numpy(np.ascontiguousarray(part))
    return part.detach().to(dev).to(torch.float32).contiguous()


class _TorchOps:
    """The two passes as float32 torch operations (device="cpu")."""

    def __init__(self, Nc, Ng, dev):
        self.Nc, self.Ng, self.dev = Nc, Ng, dev
        self.X = torch.empty((Nc, Ng), dtype=torch.float32, device=dev)
        self.bad = False

    def stage(self, blk, c0, small):
        x = torch.log(blk + torch.tensor(small, dtype=torch.float32, device=self.dev))
        self.bad |= not bool(torch.isfinite(x).all())
        self.X[c0:c0 + blk.shape[0]] = x

    def staged(self):
        """(any non-finite value, float64 column sums)"""
        if self.bad:
            return True, None
        return False, self.X.sum(0, dtype=torch.float64)

    def set_mean(self, mu32):
        self.Xc = self.X - mu32.to(self.dev)

    def apply(self, Q32):
        Y = self.Xc @ Q32.to(self.dev)
        return Y, (self.Xc.T @ Y).double().cpu()


class _HipOps:
    """The two passes on the kernels of csrc/vc_pca.hip."""

    def __init__(self, Nc, Ng, dev):
        from .engine import HipEngineError
        self.err = HipEngineError
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise HipEngineError("velocycle_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.Nc, self.Ng, self.dev = Nc, Ng, dev
        self.X = torch.empty((Nc, Ng), dtype=torch.float32, device=dev)
        self.colsum = torch.zeros(Ng, dtype=torch.float64, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(int(self.lib.vc_pca_apply_workspace(Nc, Ng, 0)), dtype=torch.float32, device=dev)
        self.Y = torch.empty((Nc, BLOCK), dtype=torch.float32, device=dev)
        self.Z = torch.empty((Ng, BLOCK), dtype=torch.float64, device=dev)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _check(self, rc, what):
        if rc != _lib.VC_OK:
            raise self.err(f"{what} failed ({rc}): {self.lib.vc_last_error(None).decode()}")

    def stage(self, blk, c0, small):
        n = blk.shape[0]
        partial = torch.empty(((n + 63) // 64, self.Ng), dtype=torch.float64, device=self.dev)
        self._check(self.lib.vc_pca_stage(C.c_void_p(blk.data_ptr()), n, self.Ng, self.Ng, C.c_float(small),
                                          C.c_void_p(self.X[c0].data_ptr()), self.Ng, C.c_void_p(self.colsum.data_ptr()),
                                          C.c_void_p(partial.data_ptr()), C.c_void_p(self.flag.data_ptr()), self._stream()),
                    "vc_pca_stage")

    def staged(self):
        if int(self.flag.item()):
            return True, None
        return False, self.colsum

    def set_mean(self, mu32):
        self.mu = mu32.to(self.dev).contiguous()

    def apply(self, Q32):
        Q = Q32.to(self.dev).contiguous()
        self._check(self.lib.vc_pca_apply(C.c_void_p(self.X.data_ptr()), self.Nc, self.Ng, self.Ng, C.c_void_p(self.mu.data_ptr()),
                                          C.c_void_p(Q.data_ptr()), C.c_void_p(self.Y.data_ptr()), C.c_void_p(self.Z.data_ptr()),
                                          C.c_void_p(self.ws.data_ptr()), self.ws.numel(), 0, self._stream()), "vc_pca_apply")
        return self.Y, self.Z.cpu()


def pca_scores(layer, small_count, n_components=2, *, device, random_state=0, tol=1e-6, max_iter=200, chunk_cells=None):
    """layer: (Nc, Ng) cells x genes like an AnnData layer: numpy or torch (float32 or float64), or scipy CSR / CSC; densified per
    chunk of `chunk_cells` cells (the result does not depend on it for multiples of 64).  device: "cuda", "cuda:N" or "cpu".
    Returns a `PCAScores` record."""
    Nc, Ng = int(layer.shape[0]), int(layer.shape[1])
    n = int(n_components)
    if n < 1 or n > MAX_COMPONENTS:
        raise ValueError(f"n_components must be in 1..{MAX_COMPONENTS} on the device path, got {n_components}")
    if Ng < BLOCK:
        raise ValueError(f"the device path iterates on a block of {BLOCK} vectors and needs at least {BLOCK} genes, got {Ng}")
    if Nc < 2:
        raise ValueError(f"a principal component analysis needs at least 2 cells, got {Nc}")
    if chunk_cells is not None and int(chunk_cells) < 1:
        raise ValueError("chunk_cells must be >= 1")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    if device is None:
        raise ValueError("pca_scores needs a device ('cuda', 'cuda:N' or 'cpu')")
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
        dev = torch.device(f"cuda:{torch.cuda.current_device()}")
    step = int(chunk_cells) if chunk_cells is not None else default_chunk_cells(Ng)
    step = min(step, Nc)
    # resident: X, one chunk of raw values and its column-sum partials, Y, the workgroups' partial rows (at most 512 x Ng x 8 floats)
    need = 4 * Nc * Ng + 4 * step * Ng + 8 * ((step + 63) // 64) * Ng + 4 * Nc * BLOCK + 4 * 512 * Ng * BLOCK
    if dev.type == "cuda" and not torch.cuda.is_available():
        from .engine import HipEngineError
        raise HipEngineError("velocycle_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    free = _free_bytes(dev)
    if need > free:
        raise ValueError(f"the staged matrix does not fit the device's free memory: {Nc} x {Ng} float32 and its buffers need "
                         f"{need} bytes, {free} are free on {dev}")
    if not (hasattr(layer, "tocsr") or torch.is_tensor(layer)):
        layer = np.asarray(layer)
    elif _is_sparse(layer):
        layer = layer.tocsr()
    with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
        return _solve(layer, Nc, Ng, n, dev, step, small_count, random_state, tol, max_iter)


def _solve(layer, Nc, Ng, n, dev, step, small_count, random_state, tol, max_iter):
    ops = (_HipOps if dev.type == "cuda" else _TorchOps)(Nc, Ng, dev)
    small = float(np.float32(small_count))
    for c0 in range(0, Nc, step):
        c1 = min(Nc, c0 + step)
        blk = _dense_block(layer, c0, c1, Ng, dev)
        ops.stage(blk, c0, small)
        del blk
    bad, colsum = ops.staged()
    if bad:
        raise ValueError(f"log(layer + small_count) is not finite somewhere: every value v needs a finite v + small_count > 0 "
                         f"(small_count = {small_count})")
    mean = colsum.cpu() / Nc                                                    # float64
    ops.set_mean(mean.to(torch.float32))

    gen = torch.Generator(device="cpu").manual_seed(int(random_state))
    Q = torch.linalg.qr(torch.randn((Ng, BLOCK), generator=gen, dtype=torch.float64))[0]
    converged, residual, it = False, float("inf"), 0
    V = theta = None
    for it in range(1, int(max_iter) + 1):
        Q32 = Q.to(torch.float32)
        _, Z = ops.apply(Q32)
        Qr = Q32.double()                                                       # the block the pass has seen
        H = Qr.T @ Z
        H = 0.5 * (H + H.T)
        theta, W = torch.linalg.eigh(H)
        theta, W = theta.flip(0), W.flip(1)
        V = Qr @ W
        R = Z @ W[:, :n] - V[:, :n] * theta[:n]
        residual = float(R.norm(dim=0).max() / theta[0])
        if residual <= tol:
            converged = True
            break
        Q = torch.linalg.qr(Z)[0]
    if not converged:
        warnings.warn(f"pca_scores: the power iteration stopped at max_iter = {max_iter} with residual {residual:.3g} > tol = {tol:g}; "
                      "the components are returned as they stand", RuntimeWarning, stacklevel=3)
    top = V.abs().argmax(dim=0)                                                 # the first of equal magnitudes
    sign = torch.sign(V[top, torch.arange(BLOCK)])
    sign[sign == 0] = 1.0
    V = V * sign
    Y, _ = ops.apply(V.to(torch.float32))
    return PCAScores(pcs=Y[:, :n].clone(), components_=V[:, :n].T.contiguous().numpy(),
                     explained_variance_=(theta[:n] / (Nc - 1)).numpy(), mean_=mean.numpy(), n_iter_=it, residual_=residual,
                     converged_=converged)
