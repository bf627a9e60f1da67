"""Launcher of the Bhattacharyya similarity kernels (csrc/simscore.hip).

``dss`` -- sum |sqrt(A) sqrt(A)^T - sqrt(B) sqrt(B)^T| / n_docs over two [D, K] sets of
document-topic rows, 64 x 64 tiles of the two D x D products at a time: the only workspace
is one float64 per tile pair.  ``bhattacharyya`` -- sqrt(X) sqrt(Y)^T as a float64 [M, N]
matrix; ``tss`` -- the sum over its columns of the column maxima.  Everything is computed in
float64 on the device whatever the inputs' type, and no result depends on the grid.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import kernel_abi as abi
from . import native


def max_rows() -> int:
    """The largest K of ``dss`` and M, N of ``bhattacharyya`` (csrc/simscore.hip SS_MAX_K)."""
    return int(native.kernels().gfk_sim_max_rows())


def _operand(t: torch.Tensor, name: str) -> torch.Tensor:
    """A 2-D fp32 / fp64 CUDA tensor whose rows are contiguous (other layouts are copied)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA tensor")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, got {t.dtype}")
    if t.shape[1] and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _grid(max_grid: Optional[int]) -> int:
    if max_grid is None:
        return 0
    if int(max_grid) < 1:
        raise ValueError("max_grid must be a positive number of workgroups")
    return int(max_grid)


@torch.no_grad()
def dss(theta_true: torch.Tensor, theta: torch.Tensor, n_docs: Optional[int] = None,
        max_grid: Optional[int] = None) -> torch.Tensor:
    """Document similarity score of ``theta`` [D, Kb] against ``theta_true`` [D, Ka] as a 0-d
    float64 tensor on their device; ``n_docs``: the divisor (default D).  ``max_grid`` caps
    the persistent workgroups; the result does not depend on it."""
    a, b = _operand(theta_true, "theta_true"), _operand(theta, "theta")
    if a.device != b.device:
        raise ValueError("theta_true and theta must be on the same device")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"theta_true has {a.shape[0]} documents, theta {b.shape[0]}")
    grid = _grid(max_grid)
    D, Ka, Kb = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
    n = D if n_docs is None else int(n_docs)
    out = torch.zeros((), dtype=torch.float64, device=a.device)
    if D == 0:
        return out
    if n < 1:
        raise ValueError("n_docs must be positive")
    lib = native.kernels()
    if not 1 <= Ka <= max_rows() or not 1 <= Kb <= max_rows():
        raise ValueError(f"{Ka} / {Kb} topics: the similarity kernels take 1 to {max_rows()}")
    items = int(lib.gfk_dss_items(D))
    if items < 0:
        raise ValueError(f"{D} documents: the tile pairs do not fit an int")
    part = torch.empty(items, dtype=torch.float64, device=a.device)
    p = abi.GfkDss()
    p.a, p.b, p.part, p.out = a.data_ptr(), b.data_ptr(), part.data_ptr(), out.data_ptr()
    p.lda, p.ldb, p.n_docs, p.part_len = a.stride(0), b.stride(0), n, items
    p.D, p.Ka, p.Kb = D, Ka, Kb
    p.a_f64, p.b_f64 = int(a.dtype == torch.float64), int(b.dtype == torch.float64)
    p.max_grid = grid
    with torch.cuda.device(a.device):
        rc = lib.gfk_dss(C.byref(p), torch.cuda.current_stream(a.device).cuda_stream)
    if rc:
        raise RuntimeError(f"gfk_dss failed ({rc})")
    return out


def _bc(x, y, max_grid, want_tss: bool):
    x, y = _operand(x, "x"), _operand(y, "y")
    if x.device != y.device:
        raise ValueError("both operands must be on the same device")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"rows of {x.shape[1]} and {y.shape[1]} entries cannot be compared")
    grid = _grid(max_grid)
    M, N, L = int(x.shape[0]), int(y.shape[0]), int(x.shape[1])
    bc = torch.zeros(M, N, dtype=torch.float64, device=x.device)
    tss_out = torch.zeros((), dtype=torch.float64, device=x.device) if want_tss else None
    if want_tss and N and not M:
        raise ValueError("tss needs at least one learned topic")
    if not M or not N or not L:                 # empty sums
        return bc, tss_out
    lib = native.kernels()
    if M > max_rows() or N > max_rows():
        raise ValueError(f"{M} x {N} rows: the similarity kernels take at most {max_rows()} each")
    part_len = int(lib.gfk_bc_ranges(L)) * M * N
    part = torch.empty(part_len, dtype=torch.float64, device=x.device)
    p = abi.GfkBc()
    p.x, p.y, p.part, p.bc = x.data_ptr(), y.data_ptr(), part.data_ptr(), bc.data_ptr()
    p.tss = tss_out.data_ptr() if want_tss else None
    p.ldx, p.ldy, p.part_len = x.stride(0), y.stride(0), part_len
    p.M, p.N, p.L = M, N, L
    p.x_f64, p.y_f64 = int(x.dtype == torch.float64), int(y.dtype == torch.float64)
    p.max_grid = grid
    with torch.cuda.device(x.device):
        rc = lib.gfk_bc(C.byref(p), torch.cuda.current_stream(x.device).cuda_stream)
    if rc:
        raise RuntimeError(f"gfk_bc failed ({rc})")
    return bc, tss_out


@torch.no_grad()
def bhattacharyya(x: torch.Tensor, y: torch.Tensor, max_grid: Optional[int] = None) -> torch.Tensor:
    """``BC[i][j] = sum_l sqrt(x[i][l] y[j][l])`` of ``x`` [M, L] and ``y`` [N, L] as a float64
    [M, N] tensor on their device."""
    return _bc(x, y, max_grid, False)[0]


@torch.no_grad()
def tss(betas: torch.Tensor, topic_vectors: torch.Tensor, max_grid: Optional[int] = None) -> torch.Tensor:
    """Topic similarity score: the sum over the ground-truth ``topic_vectors`` [N, V] of the best
    Bhattacharyya coefficient with a row of ``betas`` [M, V], as a 0-d float64 tensor."""
    return _bc(betas, topic_vectors, max_grid, True)[1]
