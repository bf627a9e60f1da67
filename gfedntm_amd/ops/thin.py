"""Token-wise thinning of a CSR corpus (csrc/thin.hip) and its numpy twin.

Every token of a non-zero (document d, word w, count x) is kept with the non-zero's
probability p, decided by a Philox draw keyed by (seed, d, w, token): token j uses
component ``j & 3`` of ``rng4(seed, step=d, tag=RNG_THIN | ((j >> 2) << 8), idx=w)``
through ``u01`` and is kept iff ``u < p`` in fp32.  The kept count is an exact
Binomial(x, p) that no grid, chunking or engine changes.

* :func:`split` -- a constant rate: ``(kept, rest)`` with ``kept + rest == X``
  (document completion: ``TopicModelBase.score(..., completion=rate)``).  The two engines
  agree exactly: ``u01`` and the rate are exact in fp32.
* :func:`thin_by_topic` -- p = theta[d, e] tw[e, w] / sum_k theta[d, k] tw[k, w], the
  responsibility of topic e for the token (the HTM-WS submodel corpus).  Bitwise
  reproducible within an engine; across engines p agrees to fp32 rounding (the kernel
  contracts the k-sum into FMAs and divides with the hardware reciprocal), so a draw
  that falls between the two values of p may differ.

``engine``: ``"fused"`` (the kernels; raises off-GPU or without the kernel library),
``"host"`` (numpy), ``None`` (fused for a :class:`DeviceCSR` on a GPU, host otherwise).
A :class:`DeviceCSR` comes back as DeviceCSRs on its device (contextual / label tensors
shared), anything else as scipy CSR matrices -- except under ``engine="fused"``, which
uploads it and returns DeviceCSRs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import scipy.sparse as sp
import torch

from ..data.bow import DeviceCSR, to_csr
from . import kernel_abi as abi
from . import native

RNG_THIN = 6                 # csrc/gfk_common.h
MAX_COUNT = 65535            # tokens per non-zero: the block index stays below 2^14
HOST_SLAB = 1 << 20          # Philox blocks / non-zeros per numpy slab
DOC_CHUNK = 1 << 20          # default documents per launch

_U32 = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------- numpy twin
def philox4x32_10(seed: int, c0, c1, c2, c3):
    """csrc/gfk_common.h philox(): 10 rounds, key (seed lo, seed hi); four uint64 arrays
    holding 32-bit words."""
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    shape = np.broadcast(np.asarray(c0), np.asarray(c1), np.asarray(c2), np.asarray(c3)).shape
    x = [np.broadcast_to(np.asarray(v, dtype=np.uint64), shape).copy() for v in (c0, c1, c2, c3)]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x[0]
        p1 = np.uint64(0xCD9E8D57) * x[2]
        x = [((p1 >> np.uint64(32)) ^ x[1] ^ k0) & _U32, p1 & _U32,
             ((p0 >> np.uint64(32)) ^ x[3] ^ k1) & _U32, p0 & _U32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _U32
    return x


def host_draws(seed: int, doc, word, x, p) -> np.ndarray:
    """Kept tokens [nnz] (int32) of non-zeros (global document ``doc``, word ``word``,
    count ``x``) at keep probabilities ``p`` (compared in fp32): the kernel's draws."""
    seed = int(seed) % (1 << 64)
    doc, word = np.asarray(doc, dtype=np.int64), np.asarray(word, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    p = np.asarray(p, dtype=np.float32)
    kept = np.where(p >= 1.0, x, 0).astype(np.int32)
    live = np.flatnonzero((p > 0.0) & (p < 1.0) & (x > 0))
    nb = (x[live] + 3) >> 2                       # Philox blocks of four tokens
    cum = np.cumsum(nb)
    a = 0
    while a < len(live):
        base = int(cum[a - 1]) if a else 0
        b = max(int(np.searchsorted(cum, base + HOST_SLAB, side="right")), a + 1)
        sel, nbs = live[a:b], nb[a:b]
        owner = np.repeat(np.arange(len(sel)), nbs)
        jb = np.arange(int(nbs.sum()), dtype=np.int64) - (np.cumsum(nbs) - nbs)[owner]
        r = philox4x32_10(seed, word[sel][owner], doc[sel][owner], RNG_THIN | (jb << 8), 0x5EED)
        xs, ps = x[sel][owner], p[sel][owner]
        hit = np.zeros(len(owner), dtype=np.int64)
        for c in range(4):
            u = (r[c] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
            hit += (4 * jb + c < xs) & (u < ps)
        kept[sel] = np.bincount(owner, weights=hit, minlength=len(sel)).astype(np.int32)
        a = b
    return kept


def host_responsibility(rows, cols, thetas, topic_word, topic: int) -> np.ndarray:
    """p [nnz] in fp32, the k-sum in the kernel's order (even and odd topics apart)."""
    th = np.asarray(thetas, dtype=np.float32)
    tw = np.asarray(topic_word, dtype=np.float32)
    K = th.shape[1]
    out = np.empty(len(rows), dtype=np.float32)
    for a in range(0, len(rows), HOST_SLAB):
        r, c = rows[a:a + HOST_SLAB], cols[a:a + HOST_SLAB]
        z0 = np.zeros(len(r), dtype=np.float32)
        z1 = np.zeros(len(r), dtype=np.float32)
        for k in range(0, K - 1, 2):
            z0 += th[r, k] * tw[k, c]
            z1 += th[r, k + 1] * tw[k + 1, c]
        if K & 1:
            z0 += th[r, K - 1] * tw[K - 1, c]
        den, num = z0 + z1, th[r, topic] * tw[topic, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(den > 0, np.where(num >= den, np.float32(1), num / den), np.float32(0))
        out[a:a + HOST_SLAB] = np.clip(p, 0, 1)
    return out


def _compact(indptr, indices, vals, n_docs):
    rows = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(indptr))
    on = vals > 0
    ptr = np.zeros(n_docs + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows[on], minlength=n_docs), out=ptr[1:])
    return ptr, indices[on].astype(np.int32), vals[on].astype(np.float32)


# --------------------------------------------------------------------------- plumbing
def _engine(engine, data) -> str:
    if engine not in (None, "fused", "host"):
        raise ValueError("engine must be None, 'fused' or 'host'")
    on_gpu = isinstance(data, DeviceCSR) and data.device.type == "cuda"
    if engine is None:
        return "fused" if on_gpu else "host"
    if engine == "fused" and isinstance(data, DeviceCSR) and not on_gpu:
        raise RuntimeError("engine='fused' needs the corpus on a GPU")
    if engine == "fused" and not torch.cuda.is_available():
        raise RuntimeError("engine='fused' needs a GPU")
    return engine


def _host_csr(data):
    if isinstance(data, DeviceCSR):
        return (data.indptr.cpu().numpy(), data.indices.cpu().numpy(), data.values.cpu().numpy(),
                (int(data.n_docs), int(data.vocab_size)))
    m = to_csr(data)
    if m.nnz >= 2**31:
        raise ValueError("shard too large for int32 CSR offsets; split it")
    return m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data, m.shape


def _bad_counts():
    return ValueError(f"counts must be integers in 0..{MAX_COUNT} (and the CSR well formed)")


def _wrap(data, parts, shape):
    """numpy (indptr, indices, values) -> the caller's kind of corpus."""
    if isinstance(data, DeviceCSR):
        t = [torch.from_numpy(np.ascontiguousarray(p)).to(data.device) for p in parts]
        return DeviceCSR.from_tensors(*t, shape, data.contextual, data.labels)
    return sp.csr_matrix((parts[2], parts[1], parts[0]), shape=shape)


def _host(data, seed, rate, thetas, topic_word, topic, want_rest, return_p):
    indptr, indices, values, shape = _host_csr(data)
    n = int(shape[0])
    if np.any((values != np.floor(values)) | (values < 0) | (values > MAX_COUNT)):
        raise _bad_counts()
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    if thetas is None:
        p = np.full(len(indices), rate, dtype=np.float32)
    else:
        p = host_responsibility(rows, indices.astype(np.int64), _np(thetas), _np(topic_word), topic)
    x = values.astype(np.int64)
    kept = host_draws(seed, rows, indices, x, p)
    out = [_wrap(data, _compact(indptr, indices, kept, n), shape)]
    if want_rest:
        out.append(_wrap(data, _compact(indptr, indices, x - kept, n), shape))
    if return_p:
        out.append(torch.from_numpy(p).to(data.device) if isinstance(data, DeviceCSR) else p)
    return out


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


@torch.no_grad()
def _fused(data, seed, rate, thetas, topic_word, topic, want_rest, return_p, chunk, max_grid=None):
    lib = native.kernels()
    if not isinstance(data, DeviceCSR):
        data = DeviceCSR(data, "cuda")
    dev = data.device
    n, V, nnz = int(data.n_docs), int(data.vocab_size), int(data.indices.numel())
    chunk = DOC_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be a positive number of documents")
    if max_grid is not None and int(max_grid) < 1:
        raise ValueError("max_grid must be a positive number of workgroups")
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    if nnz:
        v, ix, ip = data.values, data.indices, data.indptr
        bad = ((v != v.floor()) | (v < 0) | (v > MAX_COUNT) | (ix < 0) | (ix >= V)).any() \
            | (ip[0] != 0) | (ip[-1] != nnz) | (ip[1:] < ip[:-1]).any()
        if bool(bad.item()):                      # the one reduction (and sync) of the checks
            raise _bad_counts()
    th = tw = None
    K = ld = 0
    if thetas is not None:
        th = torch.as_tensor(thetas, **f32).contiguous()
        tw = torch.as_tensor(topic_word, **f32)
        if tw.dim() != 2 or tw.stride(1) != 1:
            tw = tw.contiguous()
        K, ld = int(tw.shape[0]), int(tw.stride(0)) if tw.shape[0] > 1 else int(tw.shape[1])
        if K > int(lib.gfk_thin_max_topics()):
            raise ValueError(f"K = {K}: the thinning kernels take at most {lib.gfk_thin_max_topics()} topics")
    n_parts = 2 if want_rest else 1
    p_out = torch.empty(nnz, **f32) if return_p else None
    if not nnz or not n:
        empty = [DeviceCSR.from_tensors(torch.zeros(n + 1, **i32), torch.empty(0, **i32),
                                        torch.empty(0, **f32), (n, V), data.contextual, data.labels)
                 for _ in range(n_parts)]
        return empty + ([p_out] if return_p else [])
    ws = torch.empty(nnz, **i32)
    cnt = torch.empty(n_parts, n, **i32)

    def launch(pass_, outs=None, ptrs=None):
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for d0 in range(0, n, chunk):
                p = abi.GfkThin()
                p.indptr = data.indptr.data_ptr() + 4 * d0
                p.indices, p.values = data.indices.data_ptr(), data.values.data_ptr()
                p.kept = ws.data_ptr()
                p.seed, p.doc0 = int(seed) % (1 << 64), d0
                p.n_docs, p.V, p.pass_ = min(n, d0 + chunk) - d0, V, pass_
                p.max_grid = 0 if max_grid is None else int(max_grid)
                if pass_ == abi.THIN_COUNT:
                    p.n_kept = cnt[0].data_ptr() + 4 * d0
                    p.n_rest = cnt[1].data_ptr() + 4 * d0 if want_rest else None
                    p.p_out = p_out.data_ptr() if return_p else None
                    if th is not None:
                        p.theta, p.tw = th.data_ptr() + 4 * d0 * K, tw.data_ptr()
                        p.K, p.ld, p.topic = K, ld, int(topic)
                    else:
                        p.rate = float(rate)
                else:
                    p.kept_ptr = ptrs[0].data_ptr() + 4 * d0
                    p.kept_idx, p.kept_val = outs[0][0].data_ptr(), outs[0][1].data_ptr()
                    if want_rest:
                        p.rest_ptr = ptrs[1].data_ptr() + 4 * d0
                        p.rest_idx, p.rest_val = outs[1][0].data_ptr(), outs[1][1].data_ptr()
                rc = lib.gfk_thin(C.byref(p), stream)
                if rc:
                    raise RuntimeError(f"gfk_thin failed ({rc})")

    launch(abi.THIN_COUNT)
    ptr = torch.zeros(n_parts, n + 1, **i32)
    ptr[:, 1:] = torch.cumsum(cnt, 1, dtype=torch.int32)          # the outputs' row offsets
    totals = ptr[:, -1].tolist()
    outs = [(torch.empty(max(t, 1), **i32), torch.empty(max(t, 1), **f32)) for t in totals]
    launch(abi.THIN_COMPACT, outs, ptr)
    res = [DeviceCSR.from_tensors(ptr[i], outs[i][0][:t], outs[i][1][:t], (n, V),
                                  data.contextual, data.labels) for i, t in enumerate(totals)]
    return res + ([p_out] if return_p else [])


# --------------------------------------------------------------------------- public
def split(data, rate: float, seed: int, engine: Optional[str] = None, chunk: Optional[int] = None,
          max_grid: Optional[int] = None):
    """``(kept, rest)``: every token lands in ``kept`` with probability ``rate`` and in
    ``rest`` otherwise; rows stay sorted and no zero is stored.  ``rate`` 0 / 1 put
    everything into one part (the other is an all-empty CSR).  ``max_grid`` (fused engine)
    caps the workgroups of both passes, so every wave walks several rows; the result does
    not depend on it."""
    rate = float(rate)
    if not 0.0 <= rate <= 1.0:
        raise ValueError("rate must lie in [0, 1]")
    rate = float(np.float32(rate))
    if _engine(engine, data) == "fused":
        kept, rest = _fused(data, seed, rate, None, None, 0, True, False, chunk, max_grid)
    else:
        kept, rest = _host(data, seed, rate, None, None, 0, True, False)
    return kept, rest


def thin_by_topic(data, thetas, topic_word, topic: int, seed: int, engine: Optional[str] = None,
                  chunk: Optional[int] = None, return_p: bool = False,
                  max_grid: Optional[int] = None):
    """The tokens of ``data`` that topic ``topic`` is responsible for: Binomial(x_dw,
    theta[d, topic] tw[topic, w] / sum_k theta[d, k] tw[k, w]) of every non-zero.
    ``thetas`` [D, K], ``topic_word`` [K, V] (row-major; a column slice of a wider matrix
    keeps its row stride on the fused engine).  ``return_p``: also the responsibilities,
    one per non-zero of ``data`` in storage order.  ``max_grid``: as in :func:`split`."""
    n = int(data.n_docs if isinstance(data, DeviceCSR) else data.shape[0])
    V = int(data.vocab_size if isinstance(data, DeviceCSR) else data.shape[1])
    if len(thetas.shape) != 2 or len(topic_word.shape) != 2 or thetas.shape[0] != n \
            or thetas.shape[1] != topic_word.shape[0] or topic_word.shape[1] != V:
        raise ValueError(f"thetas must be [{n}, K] and topic_word [K, {V}]")
    if not 0 <= int(topic) < thetas.shape[1]:
        raise ValueError(f"topic {topic} out of range")
    if _engine(engine, data) == "fused":
        out = _fused(data, seed, 0.0, thetas, topic_word, int(topic), False, return_p, chunk,
                     max_grid)
    else:
        out = _host(data, seed, 0.0, thetas, topic_word, int(topic), False, return_p)
    return tuple(out) if return_p else out[0]
