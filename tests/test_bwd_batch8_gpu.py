"""The 8-wave ProdLDA tile backward of batched launches (stage bit 23, GFEDNTM_BWD_WAVES;
csrc/prodlda.hip prodlda_bwd8_kernel) against the 16-wave one it stands in for.  Every output
element keeps its arithmetic, so the golden is the same production loop (run_distributed on one
rank, the pattern of test_shared_reads_gpu.py) with the knob at 16: every client's flat buffer
(parameters and BN buffers), both Adam moments and the loss history, bit for bit.

Shapes, the smallest that can break it: one k tile, a ragged one and all four (K = 16 / 50 /
64); one partial vocabulary tile (V = 40) and four tiles with a last one of 8 columns
(V = 200); 129 documents at batch 64 (batches of 64, 64 and 1 and the epoch wrap), a few of
them empty; shared reads on and off; one and four rounds per graph.  Gradient mode has no
batched launch (the generic optimizer is not batched), so it runs the one-client form of the
same instance with the bit set in the engine's own descriptor.
"""
import socket

import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

BATCH, DOCS, ROUNDS = 64, 129, 8


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


_CORPORA = {}


def _corpora(n, V, seed=21):
    """129 documents per client over flat topics (beta = 1: all V words occur), rows 5, 64
    and 128 of every client empty (one in each of the first two batches, and the lone row of
    the third)."""
    if (n, V) not in _CORPORA:
        sc = generate_synthetic(vocab_size=V, n_topics=8, beta=1.0, n_docs=DOCS, n_nodes=n,
                                frozen_topics=2, nwords=(40, 60), seed=seed)
        for i in range(n):
            c = sc.counts[i].tolil()
            for r in (5, 64, 128):
                c[r] = 0
            sc.counts[i] = c.tocsr()
            sc.counts[i].eliminate_zeros()
            assert sc.counts[i].shape[0] == DOCS
        _CORPORA[(n, V)] = [ClientCorpus(synthetic=sc, node=i) for i in range(n)]
    return _CORPORA[(n, V)]


def _run(monkeypatch, corpora, params, waves, shared="auto", rpg="4"):
    from gfedntm_amd.federation.hierarchical import run_distributed_multi
    ids = list(range(1, len(corpora) + 1))
    with monkeypatch.context() as mp:
        mp.setenv("GFEDNTM_BWD_WAVES", waves)
        mp.setenv("GFEDNTM_SHARED_READS", shared)
        mp.setenv("GFEDNTM_ROUNDS_PER_GRAPH", rpg)
        out = run_distributed_multi(corpora, ids, params, "avitm", max_iters=ROUNDS,
                                    backend="fused", seed=7, rehearse_1gpu=True, keep_round=True)
        torch.cuda.synchronize()
    bs = out["round"]._batched
    out["plan"] = out["round"].fold_plan
    out["flags"] = None if bs is None else int(bs._host.stage_flags)
    out["bwd"] = None if bs is None else bs.plan
    out["round"].close()
    return out


def _state(clients):
    st = []
    for c in clients:
        e = c.tm.engine
        st += [c.tm.flat.buffer.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(), e.loss_hist.clone()]
    return st


def _assert_same(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if torch.equal(x, y):
            continue
        c, kind = divmod(i, 4)
        j = int(torch.nonzero(x != y)[0])
        n = int((x != y).sum())
        raise AssertionError(f"client {c} {['param', 'exp_avg', 'exp_avg_sq', 'loss'][kind]}: {n} of "
                             f"{x.numel()} elements differ, first {j}: {float(x[j])!r} vs {float(y[j])!r}")


def _check_shape(m, K, V):
    assert (m.K, m.V, m.bmax) == (K, V, BATCH) and m.n_tiles == -(-V // 64)


# (shared reads, rounds per graph): both pairings on every shape, the crossed ones on one
@pytest.mark.parametrize("M,K,V,shared,rpg",
                         [(M, K, V, s, r) for M in (2, 8) for K in (16, 50, 64) for V in (40, 200)
                          for s, r in (("auto", "4"), ("0", "1"))]
                         + [(2, 50, 200, "auto", "1"), (2, 50, 200, "0", "4")])
def test_eight_wave_round_is_bitwise_the_sixteen_wave_round(monkeypatch, M, K, V, shared, rpg):
    from gfedntm_amd.ops.engine import STAGE_BWD_BATCH8, UPDATE_FUSED
    corpora = _corpora(M, V)
    a = _run(monkeypatch, corpora, _params(K), "8", shared, rpg)
    b = _run(monkeypatch, corpora, _params(K), "16", shared, rpg)
    _check_shape(a["clients"][0].tm.engine._m, K, V)
    assert all(c.tm.engine.update_mode == UPDATE_FUSED for c in a["clients"])
    assert a["plan"] == b["plan"] == ("shared reads + fold kernel" if shared == "auto" else "fold kernel")
    assert a["flags"] is not None and a["flags"] & STAGE_BWD_BATCH8, a["flags"]
    assert b["flags"] is not None and not b["flags"] & STAGE_BWD_BATCH8
    assert a["bwd"].endswith("prodlda_bwd 8 waves") and b["bwd"].endswith("prodlda_bwd 16 waves")
    # the knob changes one bit of the descriptor and nothing else of the plan
    assert a["flags"] ^ b["flags"] == STAGE_BWD_BATCH8
    _assert_same(_state(a["clients"]), _state(b["clients"]))
    loss = a["clients"][0].tm.engine.loss_hist[:ROUNDS].cpu().numpy()
    assert np.isfinite(loss).all() and (loss != 0).all()


def test_forced_eight_waves_without_an_instance_is_an_error(monkeypatch):
    """K = 65 has no 8-wave instance: the forced knob raises instead of running 16 waves."""
    with pytest.raises(RuntimeError, match="GFEDNTM_BWD_WAVES=8"):
        _run(monkeypatch, _corpora(2, 40), _params(65), "8")


@pytest.mark.parametrize("V", [40, 200])
@pytest.mark.parametrize("K", [16, 50, 64])
@pytest.mark.parametrize("solver", ["sgd", "adam"])
def test_one_client_form_is_bitwise_the_sixteen_wave_kernel(K, V, solver):
    """The one-client form of the instance (nothing selects it by default: the bit is set in
    the engine's own descriptor here), in gradient mode (solver = sgd: the kernel writes the
    beta gradient, the generic optimizer steps) and with the fused Adam epilogue."""
    from gfedntm_amd.data.bow import BatchPlan, DeviceCSR
    from gfedntm_amd.models import AVITM
    from gfedntm_amd.ops.engine import STAGE_BWD_BATCH8, UPDATE_FUSED, UPDATE_GRAD
    X = _corpora(2, V)[0].synthetic.counts[0]
    assert X.shape == (DOCS, V)
    states = []
    for bit in (STAGE_BWD_BATCH8, 0):
        torch.manual_seed(3)
        tm = AVITM(input_size=V, n_components=K, hidden_sizes=(K, K), batch_size=BATCH, solver=solver,
                   verbose=False, backend="fused", device="cuda")
        e = tm.engine
        assert e.update_mode == (UPDATE_FUSED if solver == "adam" else UPDATE_GRAD)
        e.bind_data(DeviceCSR(X, "cuda"), BatchPlan.build(DOCS, BATCH, ROUNDS))
        e._m.stage_flags |= bit
        _check_shape(e._m, K, V)
        for s in range(ROUNDS):
            e.step(s)
        torch.cuda.synchronize()
        assert bool(e._m.stage_flags & STAGE_BWD_BATCH8) == bool(bit)
        states.append([tm.flat.buffer.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(), e.loss_hist.clone()])
    _assert_same(*states)
    assert np.isfinite(states[0][3][:ROUNDS].cpu().numpy()).all()


def test_forced_eight_wave_round_is_bitwise_the_branch_round(monkeypatch):
    """The forced 8-wave batched round against one graph branch per client (the engines' own
    one-client kernels, which the oracle tests check): two clients, a ragged k tile, four
    vocabulary tiles, five rounds across the epoch wrap."""
    from gfedntm_amd.federation.runner import LocalFederation
    from gfedntm_amd.ops.engine import STAGE_BWD_BATCH8
    monkeypatch.setenv("GFEDNTM_BWD_WAVES", "8")
    corpora = _corpora(2, 200)
    kw = dict(device="cuda", backend="fused", seed=4)
    a = LocalFederation(corpora, _params(50), max_iters=5, round_batched=True, **kw)
    b = LocalFederation(corpora, _params(50), max_iters=5, round_batched=False, **kw)
    a.run()
    b.run()
    torch.cuda.synchronize()
    assert a._batched is not None and b._batched is None
    assert a._batched._host.stage_flags & STAGE_BWD_BATCH8
    _check_shape(a.clients[0].tm.engine._m, 50, 200)
    _assert_same(_state(a.clients), _state(b.clients))
