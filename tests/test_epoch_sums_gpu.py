"""The running epoch loss sum kept by the thread that writes ``loss_hist`` (csrc/posterior.hip
post_epoch_sum; GfkModel.epoch_idx / epoch_run / epoch_loss): both writers -- the extra
workgroup of post_bwd (one engine) and row_bwd's batch-level workgroup (batched clients,
GFEDNTM_POST_ROWS=2) -- and NeuralLDA.

Every epoch's slot is the numpy float32 left fold of ``loss_hist`` over the epoch's steps, bit
for bit (one fp32 add per step, in step order), with one step per graph replay and with four
(replays that cross an epoch end), the two bitwise equal; after a step-counter jump into the
middle of an epoch that epoch's slot continues from the fold of the steps before the jump and
the next epoch that completes in full is exact again; with the pointers null
the kernels' other outputs are what they are with them set.

Shapes: V = 300, K = 8, hidden (16, 16), batch 8, 37 documents -- 5-step epochs whose last
batch has 5 rows -- three epochs."""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan, DeviceCSR, epoch_index
from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.federation.runner import LocalFederation
from gfedntm_amd.models.avitm import AVITM
from gfedntm_amd.ops import kernel_abi as abi
from gfedntm_amd.utils.config import load_config
from tests.helpers import random_csr

pytestmark = pytest.mark.gpu

V, K, HIDDEN, BATCH, DOCS, EPOCHS = 300, 8, (16, 16), 8, 37, 3
PER_EPOCH = -(-DOCS // BATCH)
STEPS = EPOCHS * PER_EPOCH


def left_fold(x: np.ndarray) -> np.float32:
    acc = np.float32(x[0])
    for v in x[1:]:
        acc = np.float32(acc + np.float32(v))
    return acc


def expected_slots(loss_hist: np.ndarray, epoch_end: np.ndarray, first: int = 0) -> dict:
    """{epoch: fold} of the epochs whose steps all lie in [first, len(loss_hist))."""
    idx = epoch_index(epoch_end)
    out = {}
    for e in range(int(idx[-1]) + 1):
        steps = np.flatnonzero(idx == e)
        if steps[0] >= first and epoch_end[steps[-1]]:
            out[e] = left_fold(loss_hist[steps])
    return out


def assert_slots_exact(slots: np.ndarray, loss_hist: np.ndarray, epoch_end, first: int = 0):
    exp = expected_slots(loss_hist, epoch_end, first)
    assert exp, "no complete epoch to check"
    for e, want in exp.items():
        assert slots[e].tobytes() == want.tobytes(), (e, float(slots[e]), float(want))


# ---------------------------------------------------------------- one engine (post_bwd's extra)
def _engine(model):
    torch.manual_seed(11)
    X = random_csr(DOCS, V, 40, seed=2)
    tm = AVITM(input_size=V, n_components=K, model_type=model, hidden_sizes=HIDDEN,
               batch_size=BATCH, num_epochs=EPOCHS, backend="fused", device="cuda:0")
    plan = BatchPlan.build(DOCS, BATCH, STEPS, seed=4)
    tm.engine.bind_data(DeviceCSR(X, "cuda:0"), plan)
    return tm, plan


_one = {}


def _run_one(model, k, bind=True):
    """All steps of the plan on one engine, k steps per graph replay."""
    key = (model, k, bind)
    if key not in _one:
        tm, plan = _engine(model)
        e = tm.engine
        slots = torch.zeros(e.n_epochs, 3, dtype=torch.float32, device="cuda:0")
        if bind:
            e.bind_epoch_sums(slots, 1)              # (a column of a wider tensor: the stride)
        assert not e._m.stage_flags & abi.POST_ROWS2  # the loss is post_bwd's extra workgroup's
        e.enable_graph(True)
        s = 0
        while s < STEPS:
            kk = min(k, STEPS - s)
            e.step_k(s, kk)
            s += kk
        torch.cuda.synchronize()
        _one[key] = (slots.cpu().numpy(), e.loss_hist.cpu().numpy(), tm.flat.buffer.clone(),
                     e.exp_avg.clone(), plan)
    return _one[key]


@pytest.mark.parametrize("model", ["prodLDA", "LDA"])
def test_one_engine_slots_are_the_left_fold(model):
    slots, hist, _, _, plan = _run_one(model, 1)
    assert np.isfinite(hist).all() and (hist != 0).all()
    assert_slots_exact(slots[:, 1], hist, plan.epoch_end)
    assert (slots[:, 0] == 0).all() and (slots[:, 2] == 0).all()     # the neighbours' columns


def test_one_engine_replays_across_epoch_ends_equal_single_steps():
    s1, h1, f1, m1, plan = _run_one("prodLDA", 1)
    s4, h4, f4, m4, _ = _run_one("prodLDA", 4)       # steps 4..7 and 8..11 cross epoch ends
    assert_slots_exact(s4[:, 1], h4, plan.epoch_end)
    assert s1.tobytes() == s4.tobytes() and h1.tobytes() == h4.tobytes()
    assert torch.equal(f1, f4) and torch.equal(m1, m4)


@pytest.mark.parametrize("model", ["prodLDA", "LDA"])
def test_one_engine_null_pointers_leave_the_other_outputs(model):
    _, h1, f1, m1, _ = _run_one(model, 1)
    s0, h0, f0, m0, _ = _run_one(model, 1, bind=False)
    assert (s0 == 0).all()
    assert h0.tobytes() == h1.tobytes()
    assert torch.equal(f0, f1) and torch.equal(m0, m1)


def test_step_jump_into_an_epoch_then_exact_again():
    tm, plan = _engine("prodLDA")
    e = tm.engine
    slots = torch.zeros(e.n_epochs, 1, dtype=torch.float32, device="cuda:0")
    e.bind_epoch_sums(slots, 0)
    for s in range(PER_EPOCH + 2):                   # epoch 0 and two steps of epoch 1
        e.step(s)
    e.sync_step_counter(2)                           # back into the middle of epoch 0
    for s in range(2, 2 * PER_EPOCH):                # the rest of epoch 0, all of epoch 1
        e.step(s)
    torch.cuda.synchronize()
    got, hist = slots.cpu().numpy()[:, 0], e.loss_hist.cpu().numpy()
    # epoch 0 holds all its steps: the running sum was seeded with the fold of the two steps
    # before the jump, as loss_hist kept them (what a checkpoint resume restores) ...
    assert got[0].tobytes() == left_fold(hist[:PER_EPOCH]).tobytes()
    # ... and epoch 1, the next to complete in full, is exact
    assert_slots_exact(got, hist[:2 * PER_EPOCH], plan.epoch_end[:2 * PER_EPOCH], first=PER_EPOCH)
    assert got[1].tobytes() == left_fold(hist[PER_EPOCH:2 * PER_EPOCH]).tobytes()


# ------------------------------------------- two batched clients (row_bwd's batch-level workgroup)
_fed = {}


def _run_fed(monkeypatch, rpg, sums):
    key = (rpg, sums)
    if key not in _fed:
        sc = generate_synthetic(vocab_size=V, n_topics=10, n_docs=DOCS, n_nodes=2, frozen_topics=2,
                                nwords=(30, 60), seed=21)
        p = dict(load_config().training_params)
        p.update(num_epochs=EPOCHS, batch_size=BATCH, hidden_sizes=HIDDEN, n_components=K,
                 model_type="prodLDA")
        with monkeypatch.context() as mp:
            mp.setenv("GFEDNTM_POST_ROWS", "2")
            mp.setenv("GFEDNTM_ROUNDS_PER_GRAPH", str(rpg))
            mp.setenv("GFEDNTM_EPOCH_SUMS", sums)
            corpora = [ClientCorpus(synthetic=sc, node=i) for i in range(2)]
            fed = LocalFederation(corpora, p, max_iters=STEPS, round_batched=True, device="cuda",
                                  backend="fused", seed=5)
            fed.run()
            torch.cuda.synchronize()
        assert fed._batched is not None
        assert fed._batched._host.stage_flags & abi.POST_ROWS2     # row_bwd writes the loss
        assert (fed.epoch_sums is not None) == (sums == "device")
        _fed[key] = {
            "slots": None if fed.epoch_sums is None else fed.epoch_sums.slots.cpu().numpy(),
            "hist": [c.tm.engine.loss_hist.cpu().numpy() for c in fed.clients],
            "state": [c.tm.flat.buffer.clone() for c in fed.clients],
            "adam": [c.tm.engine.exp_avg.clone() for c in fed.clients],
            "ends": [c.plan.epoch_end.copy() for c in fed.clients],
            "replays": sorted(fed._rgk),
        }
    return _fed[key]


@pytest.mark.parametrize("rpg", [1, 4])
def test_batched_clients_slots_are_the_left_fold(monkeypatch, rpg):
    r = _run_fed(monkeypatch, rpg, "device")
    assert r["slots"].shape == (EPOCHS, 2)
    for i in range(2):
        assert np.isfinite(r["hist"][i]).all() and (r["hist"][i] != 0).all()
        assert_slots_exact(r["slots"][:, i], r["hist"][i], r["ends"][i])
    if rpg == 4:
        assert 4 in r["replays"]                     # four-round replays ran: they cross epoch ends


def test_batched_clients_replays_across_epoch_ends_equal_single_rounds(monkeypatch):
    a, b = _run_fed(monkeypatch, 1, "device"), _run_fed(monkeypatch, 4, "device")
    assert a["slots"].tobytes() == b["slots"].tobytes()
    for i in range(2):
        assert a["hist"][i].tobytes() == b["hist"][i].tobytes()
        assert torch.equal(a["state"][i], b["state"][i]) and torch.equal(a["adam"][i], b["adam"][i])


def test_batched_clients_null_pointers_leave_the_other_outputs(monkeypatch):
    a, b = _run_fed(monkeypatch, 4, "device"), _run_fed(monkeypatch, 4, "host")
    assert b["slots"] is None
    for i in range(2):
        assert a["hist"][i].tobytes() == b["hist"][i].tobytes()
        assert torch.equal(a["state"][i], b["state"][i]) and torch.equal(a["adam"][i], b["adam"][i])
