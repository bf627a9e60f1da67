"""Batched post_bwd, the rows of a workgroup through each phase together (stage bits 21 / 22,
GFEDNTM_POST_ROWS = 2 / 4) against the serial two-row shape (serial2, the bitwise reference):
per row the joint shapes run the serial shape's arithmetic operation for operation, so six
rounds must leave every client's flat state and loss history equal bit for bit.

The shapes are the smallest that reach each way this can go wrong: the last batch of an epoch
has nb = 1, 2, 3 or 5 rows (a workgroup with dead rows, odd nb, nb mod 4 != 0), 16 or 64 lanes
per output in the gemvs (hidden widths below and above 64 / 16), one to three hidden layers
(the dz ping-pong), the batch matrices read from L2, the MLP weights not staged, CombinedTM
and NeuralLDA."""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.federation.runner import LocalFederation
from gfedntm_amd.ops import kernel_abi as abi
from gfedntm_amd.utils.config import load_config

pytestmark = pytest.mark.gpu

ROUNDS = 6
POST_BITS = abi.POST_ROWS2 | abi.POST_JOINT | abi.POST_ROWS4

# name -> (clients, documents per client, batch size, K, hidden sizes, model, extra checks)
CASES = {
    "m2_k20_h50x50_nb1": (2, 17, 8, 20, (50, 50), "prodLDA", None),
    "m3_k50_h64_nb2": (3, 18, 8, 50, (64,), "prodLDA", None),
    "m2_k50_h32x48x40_nb3": (2, 19, 8, 50, (32, 48, 40), "prodLDA", None),
    "m3_k20_h50x50_nb5": (3, 21, 8, 20, (50, 50), "prodLDA", None),
    "m2_k256_batch_l2_nb3": (2, 67, 64, 256, (32,), "prodLDA", "batch_l2"),
    "m2_k200_unstaged_nb3": (2, 19, 8, 200, (128, 96), "prodLDA", "unstaged"),
    "m2_ctm_k20_nb1": (2, 17, 8, 20, (50, 50), "ctm", None),
    "m3_lda_k50_nb5": (3, 21, 8, 50, (64,), "LDA", None),
}

_runs = {}


def _run(case, knob, monkeypatch):
    """Six batched rounds of the case under GFEDNTM_POST_ROWS=knob: per client (flat state,
    loss history), and the batched launch's host descriptor."""
    M, docs, bs, K, hidden, model, _ = CASES[case]
    monkeypatch.setenv("GFEDNTM_POST_ROWS", knob)
    sc = generate_synthetic(vocab_size=300, n_topics=10, n_docs=docs, n_nodes=M, frozen_topics=2,
                            nwords=(30, 60), seed=21)
    p = dict(load_config().training_params)
    p.update(num_epochs=4, batch_size=bs, hidden_sizes=hidden, n_components=K)
    kw = dict(device="cuda", backend="fused", seed=5)
    emb = [None] * M
    if model == "ctm":
        rng = np.random.default_rng(21)
        emb = [rng.standard_normal((docs, 16)).astype(np.float32) for _ in range(M)]
        p.update(contextual_size=16)
        kw.update(model_type="ctm")
    else:
        p.update(model_type=model)
    corpora = [ClientCorpus(synthetic=sc, node=i, embeddings=emb[i]) for i in range(M)]
    fed = LocalFederation(corpora, p, max_iters=ROUNDS, round_batched=True, **kw)
    fed.run()
    torch.cuda.synchronize()
    assert fed._batched is not None
    out = [(c.tm.flat.buffer.clone(), c.tm.engine.loss_hist[:ROUNDS].clone()) for c in fed.clients]
    return out, fed._batched._host


def _reference(case, monkeypatch):
    if case not in _runs:
        _runs[case] = _run(case, "serial2", monkeypatch)
    return _runs[case]


@pytest.mark.parametrize("knob", ["2", "4"])
@pytest.mark.parametrize("case", list(CASES))
def test_joint_rows_equal_serial_rows_bitwise(monkeypatch, case, knob):
    ref, ref_host = _reference(case, monkeypatch)
    assert ref_host.stage_flags & POST_BITS == abi.POST_ROWS_SHAPES["serial2"]
    got, host = _run(case, knob, monkeypatch)
    # the forced shape really ran, on the plan the case is about
    assert host.stage_flags & POST_BITS == abi.POST_ROWS_SHAPES[knob]
    assert host.stage_flags & 3 == ref_host.stage_flags & 3
    check = CASES[case][6]
    if check == "batch_l2":
        assert host.stage_flags & 2                # batch_in_lds false
    elif check == "unstaged":
        assert host.stage_flags & 1 == 0
    else:
        assert host.stage_flags & 3 == 1           # matrices and weights in LDS
    assert all(np.isfinite(l.cpu().numpy()).all() for _, l in ref)
    for (state, loss), (rstate, rloss) in zip(got, ref):
        assert torch.equal(loss, rloss)
        assert torch.equal(state, rstate)


@pytest.mark.parametrize("knob", ["2", "4"])
def test_joint_rows_are_deterministic(monkeypatch, knob):
    a, _ = _run("m3_k50_h64_nb2", knob, monkeypatch)
    b, _ = _run("m3_k50_h64_nb2", knob, monkeypatch)
    for (sa, la), (sb, lb) in zip(a, b):
        assert torch.equal(sa, sb) and torch.equal(la, lb)
