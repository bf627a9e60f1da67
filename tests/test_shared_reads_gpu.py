"""Batched clients on one rank reading ONE shared copy of the shared prefix (GfkModel.off_own,
federation/rank_round.py MultiClientRound, GFEDNTM_SHARED_READS): the kernels read the shared
parameters and BN buffers from the copy S and store into the clients' own buffers, and the
fold kernel (csrc/comm.hip) writes the client-order sum to S alone -- to every client's buffer
too after the last round of a replay the host may look behind.  The golden is the same
production loop (run_distributed, one rank) with the knob at 0: every client's flat buffer,
Adam moments and losses bit for bit.  Reference round: server.py:477-521.
"""
import socket

import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

NEW_PLAN = "shared reads + fold kernel"
BATCH = 16


@pytest.fixture(scope="module", autouse=True)
def _one_rank_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _params(K, **kw):
    p = dict(load_config().training_params)
    p.update(num_epochs=3, batch_size=BATCH, hidden_sizes=(K, K), n_components=K)
    p.update(kw)
    return p


def _corpora(n, K=20, C=0, seed=21):
    """Uneven shards of 34 + 2 i documents: three rounds per epoch, a partial last batch of
    another size on every client, different FedAvg weights.  Flat topics (beta = 1), so the
    ~230 words all occur: four vocabulary tiles, the last one partial."""
    sc = generate_synthetic(vocab_size=230, n_topics=K, beta=1.0, n_docs=34 + 2 * (n - 1),
                            n_nodes=n, frozen_topics=2, nwords=(40, 60), seed=seed)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nd = 34 + 2 * i
        sc.counts[i] = sc.counts[i][:nd]
        sc.doc_topics[i] = sc.doc_topics[i][:nd]
        emb = rng.standard_normal((nd, C)).astype(np.float32) if C else None
        out.append(ClientCorpus(synthetic=sc, node=i, embeddings=emb))
    return out


def _run(monkeypatch, corpora, params, knob, iters=8, rpg="4", model_type="avitm", env=None,
         write_after=None):
    """run_distributed on the one-rank group; ``write_after``: after that round every client's
    shared state is overwritten on the host (the same perturbed copy everywhere; scaled, so
    the zero padding between the tensors stays zero, as in any state a host would load)."""
    from gfedntm_amd.federation import client as client_mod
    from gfedntm_amd.federation.hierarchical import run_distributed_multi
    end_round = client_mod.FederatedClient.end_round

    def end_round_and_write(self, it):
        done = end_round(self, it)
        if it == write_after:
            self.shared.mul_(1.0 + 2.0 ** -5)
        return done

    ids = list(range(1, len(corpora) + 1))
    with monkeypatch.context() as mp:
        mp.setenv("GFEDNTM_SHARED_READS", knob)
        mp.setenv("GFEDNTM_ROUNDS_PER_GRAPH", rpg)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        if write_after is not None:
            mp.setattr(client_mod.FederatedClient, "end_round", end_round_and_write)
        out = run_distributed_multi(corpora, ids, params, model_type, max_iters=iters,
                                    backend="fused", seed=7, rehearse_1gpu=True, keep_round=True)
        torch.cuda.synchronize()
    out["plan"] = out["round"].fold_plan
    out["round"].close()
    return out


def _state(out):
    st = []
    for c in out["clients"]:
        e = c.tm.engine
        st += [c.tm.flat.buffer.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(),
               e.loss_hist.clone()]
    return st


def _assert_same(a, b):
    """Bitwise equality of two runs' states; on a mismatch, name the client, buffer and
    flat-layout slot of the first differing element."""
    for i, (x, y) in enumerate(zip(_state(a), _state(b))):
        if torch.equal(x, y):
            continue
        c, kind = divmod(i, 4)
        j = int(torch.nonzero(x != y)[0])
        slot = None
        if kind < 3:
            for k, s in a["clients"][c].tm.flat.slots.items():
                if s.offset <= j < s.offset + s.numel:
                    slot = (k, j - s.offset)
        n = int((x != y).sum())
        raise AssertionError(f"client {c} {['param', 'exp_avg', 'exp_avg_sq', 'loss'][kind]}: "
                             f"{n} elements differ, first {j} {slot}: {float(x[j])!r} vs {float(y[j])!r}")


def _assert_prefixes_equal(out):
    s0 = out["clients"][0].shared
    for c in out["clients"][1:]:
        assert torch.equal(c.shared, s0)


@pytest.mark.parametrize("rpg", ["1", "4"])
@pytest.mark.parametrize("K", [20, 50])
@pytest.mark.parametrize("M", [2, 3, 8])
def test_shared_reads_are_bitwise_the_fold_kernel_plan(monkeypatch, M, K, rpg):
    """Three epochs of three rounds (partial last batches, uneven weights).  Four rounds per
    graph: chained ``more`` replays (S alone written), stretch ends at every epoch end and
    one-round graphs; one round per graph: every fold writes all."""
    corpora = _corpora(M, K)
    a = _run(monkeypatch, corpora, _params(K), "auto", rpg=rpg)
    b = _run(monkeypatch, corpora, _params(K), "0", rpg=rpg)
    m = a["clients"][0].tm.engine._m
    assert 192 < m.V < 256 and m.n_tiles == 4
    assert a["plan"] == NEW_PLAN and b["plan"] == "fold kernel"
    _assert_same(a, b)
    _assert_prefixes_equal(a)
    assert np.isfinite(a["clients"][0].tm.engine.loss_hist[:8].cpu().numpy()).all()


def test_shared_reads_learned_priors(monkeypatch):
    """Learned priors: vector jobs without a source read the client's gradient slot."""
    corpora = _corpora(3)
    p = _params(20, learn_priors=True)
    a = _run(monkeypatch, corpora, p, "auto")
    b = _run(monkeypatch, corpora, p, "0")
    assert a["plan"] == NEW_PLAN
    _assert_same(a, b)


@pytest.mark.parametrize("env", [{"GFEDNTM_POSTFOLD": "0"}, {"GFEDNTM_FWD_STRIP": "0"}])
def test_shared_reads_forward_variants(monkeypatch, env):
    """post_fwd launched on its own (its running statistics), and the tile forward."""
    corpora = _corpora(3)
    a = _run(monkeypatch, corpora, _params(20), "auto", env=env)
    b = _run(monkeypatch, corpora, _params(20), "0", env=env)
    assert a["plan"] == NEW_PLAN
    _assert_same(a, b)


def test_shared_reads_host_write_between_stretches(monkeypatch):
    """The host overwrites every client's shared state after an epoch end (round 2, the end of
    a stretch): the refresh before the next replay makes the rounds read it."""
    corpora = _corpora(3)
    a = _run(monkeypatch, corpora, _params(20), "auto", write_after=2)
    b = _run(monkeypatch, corpora, _params(20), "0", write_after=2)
    c = _run(monkeypatch, corpora, _params(20), "0")
    assert a["plan"] == NEW_PLAN
    _assert_same(a, b)
    assert not torch.equal(b["clients"][0].shared, c["clients"][0].shared)   # (the write took)


@pytest.mark.parametrize("model_type,kw,C", [("avitm", {"model_type": "LDA"}, 0),
                                             ("ctm", {"contextual_size": 64}, 64)])
def test_shared_reads_refused_plans_keep_the_fold_kernel(monkeypatch, model_type, kw, C):
    """NeuralLDA and CombinedTM are not converted: today's plan with the reason, and no
    descriptor of theirs ever carries an own-copy offset."""
    from gfedntm_amd.ops.engine import BatchedSteps
    corpora = _corpora(2, C=C)
    a = _run(monkeypatch, corpora, _params(20, **kw), "auto", iters=4, model_type=model_type)
    engines = [c.tm.engine for c in a["clients"]]
    if BatchedSteps.possible(engines):
        assert a["plan"].startswith("fold kernel (") and len(a["plan"]) > len("fold kernel ()")
        bs = BatchedSteps(engines)
        bs.prepare()
        assert bs.shared_reads_reason() is not None
        with pytest.raises(ValueError):
            bs.set_shared_reads(torch.empty_like(a["clients"][0].shared))
    else:
        assert a["plan"] == "per-client graph branches + fold kernel"
    assert all(c.tm.engine._m.off_own == 0 for c in a["clients"])
    _assert_prefixes_equal(a)


def _left_fold(bufs, off, n):
    s = bufs[0][off:off + n].clone()
    for b in bufs[1:]:
        s = s + b[off:off + n]
    return s


@pytest.mark.parametrize("M", [1, 2, 8, 9])
@pytest.mark.parametrize("off,n", [(0, None), (8, 1003), (4, 2)])
def test_local_fedavg_shared_copy_modes(M, off, n):
    """csrc/comm.hip modes 3 - 5 against the eager client-order left fold: the by-value
    kernel (M <= 8) and the table path (M = 9), a partial last float4 (and a range shorter
    than one), off != 0; nothing outside the range is touched."""
    from gfedntm_amd.parallel.aggregator import (LOCAL_REFRESH, LOCAL_SHARED, LOCAL_SHARED_ALL,
                                                 local_fedavg, prepare_local_fedavg)
    torch.manual_seed(M)
    total = 4099
    nn = total - off if n is None else n
    bufs = [torch.randn(total, device="cuda") * (1 + i) for i in range(M)]
    S = torch.randn(total, device="cuda")
    before, S0 = [b.clone() for b in bufs], S.clone()
    want = _left_fold(bufs, off, nn)
    prepare_local_fedavg(bufs)

    def outside_untouched(t, t0):
        return torch.equal(t[:off], t0[:off]) and torch.equal(t[off + nn:], t0[off + nn:])

    local_fedavg(bufs, LOCAL_SHARED, off=off, n=n, dst=S)
    torch.cuda.synchronize()
    assert torch.equal(S[off:off + nn], want) and outside_untouched(S, S0)
    assert all(torch.equal(b, b0) for b, b0 in zip(bufs, before))
    S.copy_(S0)
    local_fedavg(bufs, LOCAL_REFRESH, off=off, n=n, dst=S)
    torch.cuda.synchronize()
    assert torch.equal(S[off:off + nn], before[0][off:off + nn]) and outside_untouched(S, S0)
    assert all(torch.equal(b, b0) for b, b0 in zip(bufs, before))
    S.copy_(S0)
    local_fedavg(bufs, LOCAL_SHARED_ALL, off=off, n=n, dst=S)
    torch.cuda.synchronize()
    for t, t0 in zip(bufs + [S], before + [S0]):
        assert torch.equal(t[off:off + nn], want) and outside_untouched(t, t0)
