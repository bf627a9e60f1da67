"""Word mover's distance between word lists with uniform masses: exact optimal transport in
float64, one batch of independent problems at a time (csrc/wmd.hip).

``distances`` -- the ground costs ``c_ij = ||a_i - b_j||_2`` of two sets of word vectors.
``emd_uniform`` -- for every pair (list of rows, list of columns) of a cost matrix, the minimum
of ``sum f_ij c_ij`` over flows whose rows sum to 1/n and columns to 1/m.  ``pairwise_wmd`` --
their composition over index lists into one table of word vectors.

The solver is successive shortest paths with node potentials in integer flow units (g =
gcd(n, m): every source supplies m/g, every sink takes n/g, T = n m/g units): for each source in
index order, Dijkstra over the n + m nodes on the reduced costs ``max(c_ij + p_i - q_j, 0)``
(least distance first; on equal distance a source before a sink, then the lower index), the
potentials advanced by ``min(distance, delta)``, the bottleneck pushed along the path.  The value
is ``sum_i (sum_j x_ij c_ij) / T``, row sums in j order added in i order.  Every loop is bounded.

Engines: ``"host"`` is the numpy twin of the kernel, the same algorithm with the same tie rules,
vectorised per Dijkstra step; ``"device"`` runs the kernels and raises without a GPU or without
the kernel library; ``None`` picks the device for CUDA tensor inputs and the host otherwise.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_WORDS = 512                    # words per list (csrc/wmd.hip WM_MAX, gfk_wmd_max_words())
DIST_BYTES_CAP = 1 << 30           # pairwise_wmd: a larger D is built per group of lists_a
_HOST_BLOCK_BYTES = 64 << 20       # distances on the host: bytes of one [rows, Ub, dim] block


def max_words() -> int:
    """The longest list ``emd_uniform`` takes, on either engine."""
    return MAX_WORDS


# --------------------------------------------------------------------------- plumbing
def _is_cuda(t) -> bool:
    return hasattr(t, "is_cuda") and bool(t.is_cuda)


def _engine(engine, *arrays) -> str:
    if engine not in (None, "host", "device"):
        raise ValueError("engine must be None, 'host' or 'device'")
    if engine is None:
        engine = "device" if any(_is_cuda(t) for t in arrays) else "host"
    if engine == "device":
        import torch
        from . import native
        if not torch.cuda.is_available():
            raise RuntimeError("engine='device' needs a GPU")
        if not native.kernels_available():
            raise RuntimeError(f"engine='device' needs the kernel library ({native.KERNELS_SO})")
    return engine


def _grid(max_grid: Optional[int]) -> int:
    if max_grid is None:
        return 0
    if int(max_grid) < 1:
        raise ValueError("max_grid must be a positive number of workgroups")
    return int(max_grid)


def _host(t) -> np.ndarray:
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def _lists(lists, limit: int, name: str) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets [L + 1], indices) of index lists, as int32; every index in [0, limit)."""
    rows = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    for r in rows:
        if r.size > MAX_WORDS:
            raise ValueError(f"{name} holds a list of {r.size} words: at most {MAX_WORDS}")
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([r.size for r in rows], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError(f"{name} holds too many words for int32 offsets")
    idx = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= limit):
        raise ValueError(f"{name} holds an index outside [0, {limit})")
    return off.astype(np.int32), idx.astype(np.int32)


# --------------------------------------------------------------------------- the host twin
def _solve_host(c: np.ndarray) -> Tuple[float, int]:
    """(value, status) of one problem on the float64 cost matrix ``c`` [n, m]."""
    n, m = c.shape
    g = math.gcd(n, m)
    sup, dem, T = m // g, n // g, n // g * m
    inf = np.inf
    p, q = np.zeros(n), np.zeros(m)
    x = np.zeros((n, m), dtype=np.int64)
    t = np.full(m, dem, dtype=np.int64)
    for r in range(n):
        s = sup
        for _ in range(T):
            if s <= 0:
                break
            dS, dT = np.full(n, inf), np.full(m, inf)
            dS[r] = 0.0
            pS, pT = np.zeros(n, dtype=np.int64), np.zeros(m, dtype=np.int64)
            vS, vT = np.zeros(n, dtype=bool), np.zeros(m, dtype=bool)
            tgt, delta = -1, 0.0
            for _ in range(n + m):
                oS, oT = np.where(vS, inf, dS), np.where(vT, inf, dT)
                i, j = int(np.argmin(oS)), int(np.argmin(oT))
                di, dj = oS[i], oT[j]
                if not (di < inf or dj < inf):
                    break                                   # nothing reachable is left
                if di <= dj:                                # a source goes before a sink
                    vS[i] = True
                    nd = di + np.maximum((c[i] + p[i]) - q, 0.0)
                    upd = ~vT & (nd < dT)
                    dT[upd] = nd[upd]
                    pT[upd] = i
                else:
                    if t[j] > 0:
                        tgt, delta = j, dj
                        break
                    vT[j] = True
                    nd = dj - np.maximum((c[:, j] + p) - q[j], 0.0)
                    upd = ~vS & (x[:, j] > 0) & (nd < dS)
                    dS[upd] = nd[upd]
                    pS[upd] = j
            if tgt < 0:
                return float("nan"), 1
            p += np.minimum(dS, delta)
            q += np.minimum(dT, delta)
            amt, j, closed = min(s, int(t[tgt])), tgt, False
            for _ in range(n + m):
                i = int(pT[j])
                if i == r:
                    closed = True
                    break
                j = int(pS[i])
                amt = min(amt, int(x[i, j]))
            if not closed or amt <= 0:
                return float("nan"), 3
            j = tgt
            for _ in range(n + m):
                i = int(pT[j])
                x[i, j] += amt
                if i == r:
                    break
                j = int(pS[i])
                x[i, j] -= amt
            t[tgt] -= amt
            s -= amt
        if s > 0:
            return float("nan"), 2
    rows = np.cumsum(x * c, axis=1)[:, -1]                  # (cumsum: strictly in index order)
    return float(np.cumsum(rows)[-1] / T), 0


def _emd_host(dist: np.ndarray, la, lb) -> Tuple[np.ndarray, np.ndarray]:
    (a_off, a_idx), (b_off, b_idx) = la, lb
    La, Lb = a_off.size - 1, b_off.size - 1
    val = np.full((La, Lb), np.inf)
    status = np.zeros((La, Lb), dtype=np.int32)
    for i in range(La):
        ra = a_idx[a_off[i]:a_off[i + 1]]
        if not ra.size:
            continue
        rows = dist[ra]
        for j in range(Lb):
            cb = b_idx[b_off[j]:b_off[j + 1]]
            if cb.size:
                val[i, j], status[i, j] = _solve_host(np.ascontiguousarray(rows[:, cb]))
    return val, status


# --------------------------------------------------------------------------- the device path
def _operand(t, name: str):
    """A 2-D fp32 / fp64 CUDA tensor whose rows are contiguous (other layouts are copied)."""
    import torch
    if not torch.is_tensor(t):
        t = torch.tensor(_host(t))                  # (a copy: the array may be read-only)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D, got {tuple(t.shape)}")
    t = t.detach()
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if not t.is_cuda:
        t = t.cuda()
    if t.shape[1] and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


def _dist_device(a, b, max_grid: int):
    import torch
    from . import kernel_abi as abi
    from . import native
    a, b = _operand(a, "vec_a"), _operand(b, "vec_b")
    if a.device != b.device:
        raise ValueError("both sets of vectors must be on the same device")
    Ua, Ub, dim = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    out = torch.zeros(Ua, Ub, dtype=torch.float64, device=a.device)
    if not Ua or not Ub or not dim:
        return out
    p = abi.GfkWmdDist()
    p.a, p.b, p.out = a.data_ptr(), b.data_ptr(), out.data_ptr()
    p.lda, p.ldb, p.ldo = max(a.stride(0), dim), max(b.stride(0), dim), Ub
    p.Ua, p.Ub, p.dim = Ua, Ub, dim
    p.a_f64, p.b_f64 = int(a.dtype == torch.float64), int(b.dtype == torch.float64)
    p.max_grid = max_grid
    with torch.cuda.device(a.device):
        rc = native.kernels().gfk_wmd_dist(C.byref(p), torch.cuda.current_stream(a.device).cuda_stream)
    if rc:
        raise RuntimeError(f"gfk_wmd_dist failed ({rc})")
    return out


def _emd_device(dist, la, lb, max_grid: int, capacity: int) -> Tuple[np.ndarray, np.ndarray]:
    import torch
    from . import kernel_abi as abi
    from . import native
    (a_off, a_idx), (b_off, b_idx) = la, lb
    La, Lb = a_off.size - 1, b_off.size - 1
    n_prob = La * Lb
    if n_prob >= 2 ** 31:
        raise ValueError(f"{La} x {Lb} problems do not fit one batch")
    lib = native.kernels()
    if int(lib.gfk_wmd_max_words()) != MAX_WORDS:
        raise RuntimeError("the kernel library's word limit differs from ops/wmd.py MAX_WORDS")
    max_a, max_b = int(np.diff(a_off).max()), int(np.diff(b_off).max())
    if not max_a or not max_b:                              # empty lists only
        return np.full((La, Lb), np.inf), np.zeros((La, Lb), dtype=np.int32)
    grid = int(lib.gfk_wmd_grid(max_a, max_b, capacity, n_prob, max_grid))
    if grid < 1:
        raise ValueError(f"capacity {capacity} does not hold lists of {max(max_a, max_b)} words")
    dev = dist.device
    # the four tables in one upload, the two outputs in one download
    tab = torch.from_numpy(np.concatenate([a_off, b_off, a_idx, b_idx, np.zeros(1, np.int32)])).to(dev)
    flow_len = max(int(lib.gfk_wmd_flow_len(max_a, max_b, grid)), 8)
    flow = torch.empty(flow_len, dtype=torch.int16, device=dev)
    out = torch.empty(n_prob + (n_prob + 1) // 2, dtype=torch.float64, device=dev)
    p = abi.GfkWmd()
    p.dist = dist.data_ptr()
    base = tab.data_ptr()
    p.a_off, p.b_off = base, base + 4 * a_off.size
    p.a_idx = base + 4 * (a_off.size + b_off.size)
    p.b_idx = base + 4 * (a_off.size + b_off.size + a_idx.size)
    p.flow, p.val, p.status = flow.data_ptr(), out.data_ptr(), out.data_ptr() + 8 * n_prob
    p.ldd, p.flow_len = max(dist.stride(0), dist.shape[1]), flow_len
    p.Ua, p.Ub, p.La, p.Lb = int(dist.shape[0]), int(dist.shape[1]), La, Lb
    p.max_a, p.max_b, p.cap, p.max_grid = max_a, max_b, capacity, max_grid
    with torch.cuda.device(dev):
        rc = lib.gfk_wmd_solve(C.byref(p), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise RuntimeError(f"gfk_wmd_solve failed ({rc})")
    host = out.cpu().numpy()                                # the one copy (and sync) of the batch
    val = host[:n_prob].reshape(La, Lb).copy()
    status = host[n_prob:].view(np.int32)[:n_prob].reshape(La, Lb).copy()
    return val, status


# --------------------------------------------------------------------------- public
def distances(vec_a, vec_b, engine: Optional[str] = None, max_grid: Optional[int] = None):
    """``D[i][j] = ||vec_a[i] - vec_b[j]||_2`` of ``vec_a`` [Ua, dim] and ``vec_b`` [Ub, dim] in
    float64, in the difference form (identical rows give exactly 0.0).  ``"host"``: a numpy
    array; ``"device"``: a CUDA tensor (fp32 and fp64 inputs are read as they are)."""
    eng = _engine(engine, vec_a, vec_b)
    grid = _grid(max_grid)
    if tuple(vec_a.shape[1:]) != tuple(vec_b.shape[1:]) or len(vec_a.shape) != 2:
        raise ValueError(f"vectors of shapes {tuple(vec_a.shape)} and {tuple(vec_b.shape)} cannot be compared")
    if eng == "device":
        return _dist_device(vec_a, vec_b, grid)
    a, b = _host(vec_a).astype(np.float64), _host(vec_b).astype(np.float64)
    out = np.zeros((a.shape[0], b.shape[0]))
    step = max(1, _HOST_BLOCK_BYTES // max(1, 8 * b.shape[0] * a.shape[1]))
    for r in range(0, a.shape[0], step):
        out[r:r + step] = np.sqrt(((a[r:r + step, None, :] - b[None, :, :]) ** 2).sum(-1))
    return out


def emd_uniform(dist, lists_a: Sequence[Sequence[int]], lists_b: Sequence[Sequence[int]],
                engine: Optional[str] = None, max_grid: Optional[int] = None,
                capacity: Optional[int] = None, _trusted: bool = False) -> np.ndarray:
    """The [len(lists_a), len(lists_b)] float64 transport values between uniform masses on the
    rows ``lists_a[i]`` and the columns ``lists_b[j]`` of the ground-distance matrix ``dist``
    [Ua, Ub] (a numpy array or a tensor); ``inf`` where a list is empty.  ``dist`` must be
    finite and non-negative, a list holds at most :func:`max_words` indices (an index may
    repeat: its mass does).  ``max_grid`` caps the persistent workgroups and ``capacity`` (128
    or 512) names the kernel instance; no result depends on either."""
    eng = _engine(engine, dist)
    grid = _grid(max_grid)
    if capacity not in (None, 128, 512):
        raise ValueError("capacity must be None, 128 or 512")
    if len(dist.shape) != 2:
        raise ValueError(f"dist must be 2-D, got {tuple(dist.shape)}")
    la = _lists(lists_a, int(dist.shape[0]), "lists_a")
    lb = _lists(lists_b, int(dist.shape[1]), "lists_b")
    La, Lb = la[0].size - 1, lb[0].size - 1
    if not La or not Lb:
        return np.zeros((La, Lb))
    if eng == "device":
        import torch
        d = _operand(dist, "dist")
        if d.dtype != torch.float64:
            d = d.double()
        if not _trusted and d.numel() and bool((~torch.isfinite(d) | (d < 0)).any().item()):
            raise ValueError("dist must be finite and non-negative")      # (the one reduction)
        val, status = _emd_device(d, la, lb, grid, int(capacity or 0))
    else:
        d = _host(dist).astype(np.float64, copy=False)
        if not _trusted and d.size and not bool((np.isfinite(d) & (d >= 0)).all()):
            raise ValueError("dist must be finite and non-negative")
        val, status = _emd_host(d, la, lb)
    if status.any():
        i, j = np.argwhere(status)[0]
        raise RuntimeError(f"the transport solver left problem ({i}, {j}) with status {status[i, j]} "
                           f"({int((status != 0).sum())} of {status.size} problems failed)")
    return val


def _compact(lists) -> Tuple[np.ndarray, List[np.ndarray]]:
    """(sorted unique indices, the lists as positions in them)."""
    rows = [np.asarray(l, dtype=np.int64).reshape(-1) for l in lists]
    used = np.unique(np.concatenate(rows)) if rows else np.zeros(0, dtype=np.int64)
    return used, [np.searchsorted(used, r) for r in rows]


def pairwise_wmd(lists_a: Sequence[Sequence[int]], lists_b: Sequence[Sequence[int]], vectors,
                 engine: Optional[str] = None, max_grid: Optional[int] = None) -> np.ndarray:
    """Word mover's distances [len(lists_a), len(lists_b)] between lists of row indices into
    the word-vector table ``vectors`` [W, dim] (numpy, or a tensor: one on the GPU is gathered
    there).  Only the vectors of words that occur are gathered (and, from the host, uploaded);
    where the distance matrix of all of them would pass 1 GiB, ``lists_a`` goes in groups."""
    eng = _engine(engine, vectors)
    if len(vectors.shape) != 2:
        raise ValueError(f"vectors must be [W, dim], got {tuple(vectors.shape)}")
    W = int(vectors.shape[0])
    for name, ls in (("lists_a", lists_a), ("lists_b", lists_b)):
        _lists(ls, W, name)                                  # lengths and index ranges
    out = np.zeros((len(lists_a), len(lists_b)))
    if not len(lists_a) or not len(lists_b):
        return out
    ub, pos_b = _compact(lists_b)

    def gather(idx):
        if eng == "device":
            import torch
            if torch.is_tensor(vectors):
                return vectors.detach()[torch.from_numpy(idx).to(vectors.device)].cuda()
            return torch.tensor(_host(vectors)[idx]).cuda()
        return _host(vectors)[idx]

    vb = gather(ub)
    rows_cap = max(1, DIST_BYTES_CAP // max(1, 8 * ub.size))   # rows of D within the cap
    start = 0
    while start < len(lists_a):
        # the longest run of lists whose distinct words keep D within the cap (at least one)
        end, seen = start, set()
        while end < len(lists_a):
            more = seen | set(np.asarray(lists_a[end], dtype=np.int64).reshape(-1).tolist())
            if end > start and len(more) > rows_cap:
                break
            seen, end = more, end + 1
        ua, pos_a = _compact(lists_a[start:end])
        d = distances(gather(ua), vb, engine=eng, max_grid=max_grid)
        out[start:end] = emd_uniform(d, pos_a, pos_b, engine=eng, max_grid=max_grid, _trusted=True)
        start = end
    return out
