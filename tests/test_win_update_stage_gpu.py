"""The 6-waves-per-SIMD instance of the batched W_in update (stage bit 24, GFEDNTM_WIN_WAVES;
csrc/update.hip gfk_win_update_k<512, true, 6>) and its one-round tile staging: unconditional
clamped tile-extent and dz0 loads, the preloaded first non-zero of every row slot, LDS-only
barriers, the flat p / m / v prefetch as straight-line clamped quads.  Every output element
keeps its arithmetic, so every comparison is bit for bit: parameters and BN buffers (the flat
buffer), both Adam moments and the loss history of every client.

(a) the production MultiClientRound (run_distributed on one rank) with the knob at 6 against 8
    (the same 8-wave shape with the tile body of the 8-waves-per-SIMD instance);
(b) the batched round at 6 against one graph branch per client (the engines' own one-client
    16-wave kernels, which the oracle tests check).
The one-client engines and gradient mode never run the instance (it exists for batched
launches with fused updates only), so there is no one-client arrangement to compare.

Shapes, the smallest at which the staging can go wrong: V = 200 (four tiles, the last one of 8
columns) and V = 201 (a last block of 9 x 50 elements, no multiple of 4: the subtile layout);
K = 20, hidden (50, 50) and (64, 64); batch 64 with 70 documents per client (the second batch
has 6 rows, the rows behind them keep the first batch's tile extents) and one client of 40
documents (a partial first batch: rows 40.. of the extent table were never written); per
client an empty document, one with a single word (no word in three of the tiles) and one with
every word (64 non-zeros per tile: the scatter's loop behind the preloaded pair runs three more
times); 2 and 8 clients (XCD placement) and 3 (plain placement).
"""
import socket

import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

BATCH, DOCS, SHORT, ROUNDS, K = 64, 70, 40, 5, 20


@pytest.fixture(scope="module", autouse=True)
def _one_rank_group():
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def _params(hidden=(50, 50), **kw):
    p = dict(load_config().training_params)
    p.update(num_epochs=3, batch_size=BATCH, hidden_sizes=tuple(hidden), n_components=K)
    p.update(kw)
    return p


_CORPORA = {}


def _corpora(n, V, seed=33):
    """70 documents per client over flat topics (beta = 1: all V words occur); client 1 keeps
    its first 40 only.  Of every client row 3 is empty, row 7 holds one word and row 11 every
    word; rows 65 and 66 (the second batch) the same single word and every word."""
    if (n, V) not in _CORPORA:
        sc = generate_synthetic(vocab_size=V, n_topics=8, beta=1.0, n_docs=DOCS, n_nodes=n,
                                frozen_topics=2, nwords=(40, 60), seed=seed)
        for i in range(n):
            c = sc.counts[i].tolil()
            assert c.shape == (DOCS, V)
            c[3] = 0
            for r in (7, 65):
                c[r] = 0
                c[r, (17 * i + r) % V] = 2
            for r in (11, 66):
                c[r] = 1 + (np.arange(V) + r) % 3
            c = c.tocsr()
            c.eliminate_zeros()
            if i == 1:
                c = c[:SHORT]
            assert c[3].nnz == 0 and c[7].nnz == 1 and c[11].nnz == V
            sc.counts[i] = c
        _CORPORA[(n, V)] = [ClientCorpus(synthetic=sc, node=i) for i in range(n)]
    return _CORPORA[(n, V)]


def _run(monkeypatch, corpora, params, waves):
    from gfedntm_amd.federation.hierarchical import run_distributed_multi
    ids = list(range(1, len(corpora) + 1))
    with monkeypatch.context() as mp:
        mp.setenv("GFEDNTM_WIN_WAVES", waves)
        out = run_distributed_multi(corpora, ids, params, "avitm", max_iters=ROUNDS,
                                    backend="fused", seed=7, rehearse_1gpu=True, keep_round=True)
        torch.cuda.synchronize()
    bs = out["round"]._batched
    out["flags"] = None if bs is None else int(bs._host.stage_flags)
    out["shape"] = None if bs is None else bs.plan
    out["round"].close()
    return out


def _state(clients):
    st = []
    for c in clients:
        e = c.tm.engine
        st += [c.tm.flat.buffer.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(), e.loss_hist.clone()]
    return st


def _assert_same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if torch.equal(x, y):
            continue
        c, kind = divmod(i, 4)
        j = int(torch.nonzero(x != y)[0])
        n = int((x != y).sum())
        raise AssertionError(f"client {c} {['param', 'exp_avg', 'exp_avg_sq', 'loss'][kind]}: {n} of "
                             f"{x.numel()} elements differ, first {j}: {float(x[j])!r} vs {float(y[j])!r}")


def _check_shape(m, V, H0):
    assert (m.K, m.V, m.bmax, int(m.H[0])) == (K, V, BATCH, H0) and m.n_tiles == -(-V // 64)


@pytest.mark.parametrize("M,V,hidden", [(2, 200, (50, 50)), (3, 200, (50, 50)), (8, 200, (50, 50)),
                                        (2, 200, (64, 64)), (2, 201, (50, 50))])
def test_six_waves_round_is_bitwise_the_eight_waves_round(monkeypatch, M, V, hidden):
    from gfedntm_amd.ops.engine import STAGE_WIN_BATCH8, STAGE_WIN_WAVES6, UPDATE_FUSED
    corpora = _corpora(M, V)
    a = _run(monkeypatch, corpora, _params(hidden), "6")
    b = _run(monkeypatch, corpora, _params(hidden), "8")
    _check_shape(a["clients"][0].tm.engine._m, V, hidden[0])
    assert [c.n_docs for c in a["clients"]][:2] == [DOCS, SHORT]
    assert all(c.tm.engine.update_mode == UPDATE_FUSED for c in a["clients"])
    assert a["flags"] is not None and b["flags"] is not None
    assert a["flags"] & STAGE_WIN_BATCH8 and a["flags"] & STAGE_WIN_WAVES6
    assert b["flags"] & STAGE_WIN_BATCH8 and not b["flags"] & STAGE_WIN_WAVES6
    # the knob changes one bit of the descriptor and nothing else of the plan
    assert a["flags"] ^ b["flags"] == STAGE_WIN_WAVES6
    assert a["shape"].endswith("win_update 8-wave tiles, 6 waves per SIMD")
    assert b["shape"].endswith("win_update 8-wave tiles, 8 waves per SIMD")
    _assert_same(_state(a["clients"]), _state(b["clients"]))
    for c in a["clients"]:
        loss = c.tm.engine.loss_hist[:ROUNDS].cpu().numpy()
        assert np.isfinite(loss).all() and (loss != 0).all()


def test_forced_six_waves_without_an_instance_is_an_error(monkeypatch):
    """Hidden (80, 80) has no 6-waves-per-SIMD instance: the forced knob raises instead of
    running the other one."""
    with pytest.raises(RuntimeError, match="GFEDNTM_WIN_WAVES=6"):
        _run(monkeypatch, _corpora(2, 200), _params((80, 80)), "6")


@pytest.mark.parametrize("M,V,hidden", [(2, 200, (50, 50)), (3, 200, (64, 64)), (2, 201, (50, 50))])
def test_six_waves_round_is_bitwise_the_branch_round(monkeypatch, M, V, hidden):
    from gfedntm_amd.federation.runner import LocalFederation
    from gfedntm_amd.ops.engine import STAGE_WIN_WAVES6
    monkeypatch.setenv("GFEDNTM_WIN_WAVES", "6")
    corpora = _corpora(M, V)
    kw = dict(device="cuda", backend="fused", seed=4)
    a = LocalFederation(corpora, _params(hidden), max_iters=ROUNDS, round_batched=True, **kw)
    b = LocalFederation(corpora, _params(hidden), max_iters=ROUNDS, round_batched=False, **kw)
    a.run()
    b.run()
    torch.cuda.synchronize()
    assert a._batched is not None and b._batched is None
    assert a._batched._host.stage_flags & STAGE_WIN_WAVES6
    _check_shape(a.clients[0].tm.engine._m, V, hidden[0])
    _assert_same(_state(a.clients), _state(b.clients))
