"""Epoch summaries fed from the device epoch sums (federation/epoch_sums.py): the production
loop (run_distributed, one rank, two batched clients) emits every epoch's ``train_loss`` and
``best_loss_train`` from one copy of the slots' row per epoch-ending round.

The device sum is the fp32 left fold of the epoch's n step losses, so it differs from their
float64 sum by at most n * 2^-24 * sum|loss| (n - 1 roundings of partial sums no larger than
sum|loss|, each within 2^-24 relative); ``train_loss = (train_loss + epoch_sum) / samples`` in
float64 carries that bound through the reference recurrence.  GFEDNTM_EPOCH_SUMS=host is the
torch reduction over ``loss_hist`` and reproduces it exactly; the training state does not
depend on the knob."""
import socket

import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

V, K, HIDDEN, BATCH, EPOCHS = 300, 8, (16, 16), 8, 3


@pytest.fixture(scope="module", autouse=True)
def _one_rank_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _corpora(docs):
    sc = generate_synthetic(vocab_size=V, n_topics=10, n_docs=max(docs), n_nodes=len(docs),
                            frozen_topics=2, nwords=(30, 60), seed=21)
    out = []
    for i, nd in enumerate(docs):
        sc.counts[i] = sc.counts[i][:nd]
        sc.doc_topics[i] = sc.doc_topics[i][:nd]
        out.append(ClientCorpus(synthetic=sc, node=i))
    return out


_runs = {}


def _run(monkeypatch, docs, iters, sums):
    """run_distributed on the one-rank group.  Records every emitted summary (client, epoch,
    samples, epoch sum, train_loss after it) and every copy the reader enqueued in a round."""
    key = (tuple(docs), iters, sums)
    if key in _runs:
        return _runs[key]
    from gfedntm_amd.federation import client as client_mod
    from gfedntm_amd.federation import epoch_sums as es_mod
    from gfedntm_amd.federation.hierarchical import run_distributed_multi
    emitted, copies = [], []
    emit = client_mod.FederatedClient._emit
    enqueue = es_mod.EpochSums.enqueue

    def emit_and_record(self, epoch, samples, epoch_loss):
        emit(self, epoch, samples, epoch_loss)
        emitted.append((self.id, epoch, samples, epoch_loss, self.train_loss))

    def enqueue_and_count(self, epoch, slot):
        if self._round is not None:          # (the constructor's warm-up copy has no round)
            copies.append((self._round, epoch))
        enqueue(self, epoch, slot)

    p = dict(load_config().training_params)
    p.update(num_epochs=EPOCHS, batch_size=BATCH, hidden_sizes=HIDDEN, n_components=K,
             model_type="prodLDA")
    with monkeypatch.context() as mp:
        mp.setenv("GFEDNTM_EPOCH_SUMS", sums)
        mp.setenv("GFEDNTM_ROUNDS_PER_GRAPH", "4")
        mp.setattr(client_mod.FederatedClient, "_emit", emit_and_record)
        mp.setattr(es_mod.EpochSums, "enqueue", enqueue_and_count)
        out = run_distributed_multi(_corpora(docs), list(range(1, len(docs) + 1)), p, "avitm",
                                    max_iters=iters, backend="fused", seed=7, rehearse_1gpu=True,
                                    keep_round=True)
        torch.cuda.synchronize()
    rr = out["round"]
    assert (rr.epoch_sums is not None) == (sums == "device")
    res = {"emitted": emitted, "copies": copies, "clients": [], "state": []}
    for c in out["clients"]:
        e = c.tm.engine
        first, host_sums = 0, []
        for last in np.flatnonzero(c.plan.epoch_end):
            # the host path's formula, on the same slices of the same tensor
            host_sums.append(float(e.loss_hist[first: int(last) + 1].sum()))
            first = int(last) + 1
        res["clients"].append({"id": c.id, "hist": c.loss_history().astype(np.float64),
                               "ends": np.flatnonzero(c.plan.epoch_end), "size": c.plan.size.copy(),
                               "host_sums": host_sums, "best": float(c.tm.best_loss_train),
                               "train_loss": float(c.train_loss)})
        res["state"] += [c.tm.flat.buffer.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(),
                         e.loss_hist.clone()]
    rr.close()
    _runs[key] = res
    return res


def _check_summaries(res, exact):
    """Every client's summaries: once each, in order, against the float64 recomputation from
    the loss history (``exact``: against the host formula, bit for bit)."""
    for ci in res["clients"]:
        mine = [x for x in res["emitted"] if x[0] == ci["id"]]
        assert [x[1] for x in mine] == list(range(len(ci["ends"])))       # once, in order
        tl_ref, tl_bound, first, samples, tls, tl_bounds = 0.0, 0.0, 0, 0, [], []
        for e, last in enumerate(ci["ends"]):
            steps = ci["hist"][first: last + 1]
            samples += int(ci["size"][first: last + 1].sum())
            n = len(steps)
            _, _, got_samples, got_sum, got_tl = mine[e]
            assert got_samples == samples
            if exact:
                assert got_sum == ci["host_sums"][e]
                tl_ref = (tl_ref + ci["host_sums"][e]) / samples
                assert got_tl == tl_ref
            else:
                bound = n * 2.0 ** -24 * float(np.abs(steps).sum())
                ref = float(steps.sum())                                    # float64
                print(f"client {ci['id']} epoch {e}: sum {got_sum!r} float64 {ref!r} "
                      f"|diff| {abs(got_sum - ref):.3e} bound {bound:.3e}")
                assert abs(got_sum - ref) <= bound
                tl_ref = (tl_ref + ref) / samples
                tl_bound = (tl_bound + bound) / samples
                assert abs(got_tl - tl_ref) <= tl_bound + 1e-12 * abs(tl_ref)
            tls.append(tl_ref)
            tl_bounds.append(0.0 if exact else tl_bound + 1e-12 * abs(tl_ref))
            first = last + 1
        # (two minima differ by no more than the largest difference of their terms)
        assert abs(ci["best"] - min(tls)) <= max(tl_bounds)
        assert abs(ci["train_loss"] - tls[-1]) <= tl_bounds[-1]


def test_equal_shards_device_sums_within_the_fold_bound(monkeypatch):
    res = _run(monkeypatch, [37, 37], 15, "device")
    assert len(res["emitted"]) == 2 * EPOCHS
    _check_summaries(res, exact=False)


def test_equal_shards_host_sums_are_the_parents_formula(monkeypatch):
    res = _run(monkeypatch, [37, 37], 15, "host")
    assert len(res["emitted"]) == 2 * EPOCHS and res["copies"] == []
    _check_summaries(res, exact=True)


def test_equal_shards_state_does_not_depend_on_the_knob(monkeypatch):
    a, b = _run(monkeypatch, [37, 37], 15, "device"), _run(monkeypatch, [37, 37], 15, "host")
    assert len(a["state"]) == len(b["state"]) == 8
    for x, y in zip(a["state"], b["state"]):
        assert torch.equal(x, y)


def test_equal_shards_one_copy_per_epoch_ending_round(monkeypatch):
    res = _run(monkeypatch, [37, 37], 15, "device")
    assert res["copies"] == [(4, 0), (9, 1), (14, 2)]      # one per round, not one per client


def test_unequal_shards_every_summary_once_in_order(monkeypatch):
    # 37 and 53 documents: epochs of 5 and 7 rounds, so the epoch ends differ
    res = _run(monkeypatch, [37, 53], 21, "device")
    assert [len(c["ends"]) for c in res["clients"]] == [4, 3]
    assert len(res["emitted"]) == 7
    _check_summaries(res, exact=False)
    # one copy per distinct epoch index ending in a round
    assert res["copies"] == [(4, 0), (6, 0), (9, 1), (13, 1), (14, 2), (19, 3), (20, 2)]
