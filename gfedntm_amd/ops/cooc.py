"""Launcher of the word co-occurrence kernels (csrc/cooc.hip).

``counts[i][j]`` = number of documents of a :class:`DeviceCSR` in which ``words[i]`` and
``words[j]`` both have a stored value > 0, as an int64 ``[W, W]`` tensor on the data's
device.  The documents are processed in chunks whose bit matrix
(``W * ceil(chunk / 64)`` 64-bit words) is the only workspace; the counts are integers,
so the chunking never changes them.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from ..data.bow import DeviceCSR
from . import kernel_abi as abi
from . import native

BITS_BYTES = 256 << 20      # default cap of the bit matrix of one chunk


def max_words() -> int:
    """The largest word list the kernels take (csrc/cooc.hip CO_MAX_W)."""
    return int(native.kernels().gfk_cooc_max_words())


def default_chunk(n_words: int) -> int:
    """Documents per launch that keep the bit matrix at or below 256 MiB."""
    return max(64, BITS_BYTES // (8 * max(int(n_words), 1)) * 64)


@torch.no_grad()
def counts(data: DeviceCSR, words: torch.Tensor, chunk: Optional[int] = None,
           max_grid: Optional[int] = None) -> torch.Tensor:
    """``words``: int64 tensor of distinct, in-range vocabulary indices on ``data.device``
    (checked by the caller, eval/metrics.py).  ``max_grid`` caps the workgroups of the pack
    kernel, so each walks several groups of 64 documents (the counting kernel's 2-D grid is a
    function of the shape and stays); the counts do not depend on it."""
    lib = native.kernels()
    dev = data.device
    W, V, n = int(words.numel()), int(data.vocab_size), int(data.n_docs)
    if W > max_words():
        raise ValueError(f"{W} words: the co-occurrence kernels take at most {max_words()}")
    chunk = default_chunk(W) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be a positive number of documents")
    if max_grid is not None and int(max_grid) < 1:
        raise ValueError("max_grid must be a positive number of workgroups")
    out = torch.zeros(W, W, dtype=torch.int64, device=dev)
    if not n or not W or not data.indices.numel():      # no stored entry: nothing occurs
        return out
    slot = torch.full((V,), -1, dtype=torch.int32, device=dev)
    slot[words] = torch.arange(W, dtype=torch.int32, device=dev)
    words_cap = W * (-(-min(n, chunk) // 64))
    bits = torch.empty(words_cap, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for d0 in range(0, n, chunk):
            p = abi.GfkCooc()
            p.indptr = data.indptr.data_ptr() + 4 * d0
            p.indices, p.values = data.indices.data_ptr(), data.values.data_ptr()
            p.slot, p.bits, p.counts = slot.data_ptr(), bits.data_ptr(), out.data_ptr()
            p.n_docs, p.bits_words = min(n, d0 + chunk) - d0, words_cap
            p.W, p.V = W, V
            p.max_grid = 0 if max_grid is None else int(max_grid)
            rc = lib.gfk_cooc(C.byref(p), stream)
            if rc:
                raise RuntimeError(f"gfk_cooc failed ({rc})")
    return out
