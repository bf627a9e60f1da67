"""Epoch loss sums kept on the device, read back with one copy per epoch-ending round.

The fused step's batch-level workgroup keeps the fp32 left fold of an epoch's step losses in a
slot of its own next to ``loss_hist`` (csrc/posterior.hip post_epoch_sum, ops/engine.py
``FusedEngine.bind_epoch_sums``).  A round object (rank_round.py, runner.LocalFederation) owns
one :class:`EpochSums`: a float32 ``[n_epochs, M]`` tensor whose column i belongs to its i-th
client, so the sums of clients whose epochs end in the same round with the same index are one
contiguous row.  At such a round the first client to ask enqueues ONE non-blocking copy of
that row into a pinned ring slot and records ONE event; the rank's other clients share both.
No reduction kernel runs, and the host reads no shared state, so an epoch end neither cuts a
run of rounds per graph replay nor ends a ``more`` chain (runner.round_cuts).

``GFEDNTM_EPOCH_SUMS`` = ``device`` (default: wherever every engine of the round object offers
the slots) | ``host`` (the torch reduction over ``loss_hist`` at every epoch end, and a run of
rounds cut there).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch

RING = 64      # pinned rows: epoch-ending rounds whose copy may be in flight at once


def epoch_sums_mode() -> str:
    mode = os.environ.get("GFEDNTM_EPOCH_SUMS", "device")
    if mode not in ("device", "host"):
        raise ValueError("GFEDNTM_EPOCH_SUMS must be 'device' or 'host'")
    return mode


class EpochSums:
    """The device slots of a round object's clients, and their way to the host."""

    def __init__(self, clients: List):
        self.clients = list(clients)
        engines = [c.tm.engine for c in self.clients]
        dev = engines[0].device
        M = len(engines)
        n_epochs = max(int(e.n_epochs) for e in engines)
        self.slots = torch.zeros(max(n_epochs, 1), M, dtype=torch.float32, device=dev)
        self._pinned = torch.zeros(RING, M, dtype=torch.float32, pin_memory=True)
        self._events = [torch.cuda.Event() for _ in range(RING)]
        self._next = 0
        self._round: Optional[int] = None
        self._by_epoch: Dict[int, int] = {}      # epoch -> ring slot, within the current round
        for i, (c, e) in enumerate(zip(self.clients, engines)):
            e.bind_epoch_sums(self.slots, i)     # (re-uploads the descriptor, bumps graph_gen)
            c.attach_epoch_sums(self, i)
        # first use of the pinned copy and of an event here, not inside the round loop
        self.enqueue(0, 0)
        torch.cuda.synchronize(dev)

    @staticmethod
    def attach(clients: List) -> Optional["EpochSums"]:
        """The round object's device sums, or None where today's host path stays: the knob
        says ``host``, a torch-backend or CPU engine, an engine without the slots."""
        ok = epoch_sums_mode() == "device" and bool(clients)
        for c in clients:
            e = c.tm.engine
            ok = ok and (getattr(c, "fused", False) and hasattr(e, "bind_epoch_sums")
                         and e.device.type == "cuda" and e.plan is not None)
        if not ok:
            EpochSums.detach(clients)        # (an earlier round object may have bound them)
            return None
        return EpochSums(clients)

    @staticmethod
    def detach(clients: List):
        """Back to the host path: the clients and their engines unbound (the kernels write
        ``loss_hist`` alone again).  Summaries already queued keep their pinned row and event."""
        for c in clients:
            if c._esums is not None:
                c.attach_epoch_sums(None, 0)
            e = c.tm.engine
            if getattr(e, "epoch_sums", None) is not None:
                e.bind_epoch_sums(None)

    def enqueue(self, epoch: int, slot: int):
        """One non-blocking copy of epoch ``epoch``'s row into ring row ``slot``, one event."""
        self._pinned[slot].copy_(self.slots[epoch], non_blocking=True)
        self._events[slot].record()

    def _reclaim(self, slot: int):
        """A ring row is reused RING epoch-ending rounds later: whoever still waits on it
        (its event never polled complete) emits it first."""
        ev = self._events[slot]
        for c in self.clients:
            if any(p[3] is ev for p in c._pending):
                c.flush()

    def fetch(self, it: int, epoch: int, col: int) -> Tuple[torch.Tensor, torch.cuda.Event]:
        """Client ``col``'s sum of ``epoch``, which ended in round ``it``: (a pinned one-element
        view, the event behind its copy).  Enqueued behind whatever carries round ``it`` -- the
        slot is final by then: later steps write later epochs' slots."""
        if it != self._round:
            self._round, self._by_epoch = it, {}
        slot = self._by_epoch.get(epoch)
        if slot is None:
            slot = self._next
            self._next = (slot + 1) % RING
            self._reclaim(slot)
            self.enqueue(epoch, slot)
            self._by_epoch[epoch] = slot
        return self._pinned[slot, col:col + 1], self._events[slot]
