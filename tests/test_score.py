"""Held-out scoring on the PyTorch engine (TopicModelBase.score / perplexity) against a
float64 formula written out from the state_dict, and the validation / early-stopping path
of fit() -- all on the CPU."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BOWDataset, CTMDataset
from gfedntm_amd.models import AVITM, CombinedTM
from tests.helpers import random_csr, tiny_corpus
from tests.score_oracle import oracle_loss, oracle_perplexity, oracle_score

VOCAB = {i: str(i) for i in range(4096)}


def _with_empty_row(X, row=3):
    X = X.tolil()
    X[row, :] = 0
    X = sp.csr_matrix(X, dtype=np.float32)
    X.eliminate_zeros()
    return X


def _avitm(model_type, X, seed=0):
    torch.manual_seed(seed)
    tm = AVITM(input_size=X.shape[1], n_components=8, model_type=model_type, hidden_sizes=(16, 12),
               batch_size=32, lr=5e-3, verbose=False, device="cpu", backend="torch")
    ds = BOWDataset(X, VOCAB)
    for ep in range(2):                   # non-trivial running statistics
        tm._train_epoch(ds, seed=ep)
    return tm, ds


def _check(tm, ds, X, S, ctx=None, labels=None, kl_weight=1.0):
    n, K = X.shape[0], tm.n_components
    eps = np.random.default_rng(7).standard_normal((S, n, K)) if S else None
    got = tm.score(ds, n_samples=S, eps=eps) if S else tm.score(ds, n_samples=0)
    ref = oracle_score(tm, X, eps, ctx, labels)
    assert got["engine"] == "torch"
    assert got["kl"].shape == got["rl"].shape == (n,)
    np.testing.assert_allclose(got["kl"], ref["kl"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(got["rl"], ref["rl"], rtol=1e-4, atol=1e-2)
    ce = ref.get("ce")
    if ce is not None:
        np.testing.assert_allclose(got["ce"], ce, rtol=1e-4, atol=1e-4)
    # loss and perplexity: their definitions, on the oracle's terms and on the returned ones
    np.testing.assert_allclose(got["loss"], oracle_loss(ref["kl"], ref["rl"], kl_weight, ce,
                                                        tm.batch_size), rtol=1e-5)
    np.testing.assert_allclose(got["loss"],
                               oracle_loss(got["kl"].astype(np.float64), got["rl"].astype(np.float64),
                                           kl_weight, None if ce is None else got["ce"], tm.batch_size),
                               rtol=1e-6)
    np.testing.assert_allclose(got["perplexity"], oracle_perplexity(ref["kl"], ref["rl"], X),
                               rtol=1e-5)
    return got


@pytest.mark.parametrize("model_type", ["prodLDA", "LDA"])
@pytest.mark.parametrize("S", [0, 1, 3])
def test_avitm_score_matches_formula(model_type, S):
    X = _with_empty_row(random_csr(70, 300, 30, seed=2))
    tm, ds = _avitm(model_type, X)
    got = _check(tm, ds, X, S)
    assert got["rl"][3] == 0.0 and np.isfinite(got["kl"][3])       # the empty document
    assert tm.model.training                                        # mode restored
    if S == 0:                                                      # no draw: the shorthand agrees
        assert tm.perplexity(ds, n_samples=0) == got["perplexity"]


def test_tiny_corpus_score_and_seeded_draws():
    _, terms, shards = tiny_corpus(V=200, n_docs=60, n_nodes=1)
    X = shards[0]
    tm, ds = _avitm("prodLDA", X)
    _check(tm, ds, X, 2)
    a, b, c = tm.score(ds, seed=11), tm.score(ds, seed=11), tm.score(ds, seed=12)
    np.testing.assert_array_equal(a["rl"], b["rl"])
    np.testing.assert_array_equal(a["kl"], c["kl"])                 # KL has no draw in it
    assert not np.array_equal(a["rl"], c["rl"])
    assert 1.0 < a["perplexity"] < 10 * X.shape[1]


def test_combined_label_head_loss_bookkeeping():
    torch.manual_seed(0)
    n, V, C, L = 70, 120, 10, 4
    X = random_csr(n, V, 20, seed=4)
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((n, C)).astype(np.float32)
    labels = np.eye(L, dtype=np.float32)[rng.integers(0, L, n)]
    tm = CombinedTM(input_size=V, contextual_size=C, n_components=6, hidden_sizes=(16, 12),
                    batch_size=32, verbose=False, device="cpu", backend="torch", label_size=L,
                    loss_weights={"beta": 3.0})
    ds = CTMDataset(emb, X, VOCAB, labels=labels)
    for ep in range(2):
        tm._train_epoch(ds, seed=ep)
    got = _check(tm, ds, X, 2, ctx=emb, labels=labels, kl_weight=3.0)
    assert "ce" in got and got["ce"].shape == (n,)
    # the validation loop's number is this loss
    assert tm._validate_epoch(ds, seed=5) == (n, tm.score(ds, n_samples=1, seed=5)["loss"])
    info = tm.engine_info
    assert info["score_engine"] == "torch" and "score_fused_unavailable" in info


def test_fit_validates_every_epoch_and_stops_early():
    """Training on one half of the vocabulary, validating on the other: the validation
    loss rises as the model commits to the training words, and patience=1 stops fit()."""
    V, n = 200, 96

    def docs(lo, hi, seed):
        X = random_csr(n, hi - lo, 25, seed=seed)
        full = sp.lil_matrix((n, V), dtype=np.float32)
        full[:, lo:hi] = X
        return BOWDataset(sp.csr_matrix(full), VOCAB)

    train, val = docs(0, V // 2, 1), docs(V // 2, V, 2)
    torch.manual_seed(0)
    tm = AVITM(input_size=V, n_components=5, hidden_sizes=(16,), batch_size=32, lr=0.05,
               num_epochs=40, verbose=False, device="cpu", backend="torch")
    seen = []
    inner = tm._validate_epoch

    def spy(ds, *a, **k):
        out = inner(ds, *a, **k)
        seen.append(out[1])
        return out

    tm._validate_epoch = spy
    tm.fit(train, val, patience=1, n_samples=1)
    assert tm.early_stopping.early_stop
    assert tm.nn_epoch < tm.num_epochs - 1                          # stopped early
    assert len(seen) == tm.nn_epoch + 1                             # once per epoch
    assert all(np.isfinite(seen)) and seen[-1] > min(seen)          # ... because the loss rose
    assert tm.training_doc_topic_distributions.shape == (n, 5)
