"""Token-wise thinning on the host engine (gfedntm_amd/ops/thin.py) against a float64 oracle
of the keyed draws, document-completion scoring on the PyTorch engine against the float64
formula, and the keyed HTM-WS submodel corpus -- all on the CPU."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BOWDataset, DeviceCSR
from gfedntm_amd.experiments.tm_wrapper import TMWrapper, htm_ws_counts
from gfedntm_amd.models import AVITM
from gfedntm_amd.ops import thin
from tests.helpers import random_csr
from tests.score_oracle import _logsumexp, _softmax, np_state, oracle_moments
from tests.test_theta_infer import philox4x32_10

VOCAB = {i: str(i) for i in range(8200)}
RNG_THIN = 6


# ------------------------------------------------------------------------------ oracle
def oracle_kept(seed, rows, cols, x, p):
    """Kept tokens of every non-zero in float64: token j of (document d, word w) draws
    component j & 3 of Philox(idx = w, step = d, tag = RNG_THIN | ((j >> 2) << 8)),
    u = (word >> 8) / 2^24, and is kept iff u < p."""
    x = np.asarray(x).astype(np.int64)
    owner = np.repeat(np.arange(len(x)), x)
    j = np.arange(len(owner), dtype=np.int64) - (np.cumsum(x) - x)[owner]
    r = np.stack(philox4x32_10(seed, np.asarray(cols, dtype=np.int64)[owner],
                               np.asarray(rows, dtype=np.int64)[owner],
                               RNG_THIN | ((j >> 2) << 8), 0x5EED))
    word = r[j & 3, np.arange(len(owner))]
    u = np.floor(word.astype(np.float64) / 256) / 2**24
    hit = u < np.asarray(p, dtype=np.float64)[owner]
    return np.bincount(owner, weights=hit, minlength=len(x)).astype(np.int64)


def csr_rows(X):
    return np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))


def _part(X, vals):
    m = sp.csr_matrix((vals.astype(np.float32), X.indices.copy(), X.indptr.copy()), shape=X.shape)
    m.eliminate_zeros()
    return m


def oracle_split(X, rate, seed):
    """(kept, rest) of the oracle's draws at the fp32 value of ``rate``."""
    kept = oracle_kept(seed, csr_rows(X), X.indices, X.data,
                       np.full(X.nnz, np.float32(rate), dtype=np.float32))
    return _part(X, kept), _part(X, X.data.astype(np.int64) - kept)


def oracle_completion(tm, Xk, Xr, eps=None, ctx=None):
    """float64 (KL, RL) of document completion: the posterior of the kept part ``Xk``, the
    reconstruction term on the rest ``Xr`` (tests/score_oracle.py oracle_score, with the
    two CSRs apart)."""
    sd = np_state(tm)
    K = tm.n_components
    mu, ls = oracle_moments(tm, Xk, ctx)
    pm = tm.model.prior_mean.detach().double().cpu().numpy()
    pv = tm.model.prior_variance.detach().double().cpu().numpy()
    kl = 0.5 * ((np.exp(ls) / pv).sum(1) + ((pm - mu) ** 2 / pv).sum(1) - K
                + np.log(pv).sum() - ls.sum(1))
    beta = sd["beta"]
    rm, rv = sd["beta_batchnorm.running_mean"], sd["beta_batchnorm.running_var"]
    bn_eps = tm.model.beta_batchnorm.eps
    x = np.asarray(Xr.toarray(), dtype=np.float64)
    draws = [mu] if eps is None else [mu + np.asarray(e, dtype=np.float64) * np.exp(0.5 * ls)
                                      for e in eps]
    rl = np.zeros(len(kl))
    for z in draws:
        theta = _softmax(z)
        if tm.model.is_prodlda:
            zn = (theta @ beta - rm) / np.sqrt(rv + bn_eps)
            p = np.exp(zn - _logsumexp(zn))
        else:
            p = theta @ _softmax((beta - rm) / np.sqrt(rv + bn_eps))
        rl += -(x * np.log(p + 1e-10)).sum(1)
    return {"kl": kl, "rl": rl / len(draws)}


def planted_csr(V=700, seed=9):
    """D = 70, about 40 non-zeros per row; empty rows first and last, a row of 130
    non-zeros (three ballot rounds, the last partial), a row holding one token, and counts
    9 and 37 (several Philox blocks of four tokens, one partial)."""
    X = random_csr(70, V, 40, seed=seed).tolil()
    rng = np.random.default_rng(3)
    X[0, :] = 0
    X[69, :] = 0
    X[2, :] = 0
    X[2, rng.choice(V, 130, replace=False)] = rng.integers(1, 5, 130)
    X[4, :] = 0
    X[4, V - 1] = 1
    X[6, 11] = 9
    X[6, 300] = 37
    X = sp.csr_matrix(X, dtype=np.float32)
    X.eliminate_zeros()
    X.sort_indices()
    assert X[0].nnz == 0 and X[69].nnz == 0 and X[2].nnz == 130 and X[4].sum() == 1
    return X


def assert_same_csr(a, b):
    for name in ("indptr", "indices", "data"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


# ------------------------------------------------------------------------------ split
@pytest.mark.parametrize("rate", [0.3, 0.5])
def test_host_split_equals_oracle(rate):
    X = planted_csr()
    kept, rest = thin.split(X, rate, seed=0x5EED_1234, engine="host")
    ok, orr = oracle_split(X, rate, 0x5EED_1234)
    assert_same_csr(kept, ok)
    assert_same_csr(rest, orr)
    assert kept.has_sorted_indices and (kept.data > 0).all() and (rest.data > 0).all()
    assert (kept + rest != X).nnz == 0
    assert 0 < kept.sum() < X.sum()
    # a 64-bit seed reaches both key words
    k2, _ = thin.split(X, rate, seed=(7 << 32) | 5, engine="host")
    assert_same_csr(k2, oracle_split(X, rate, (7 << 32) | 5)[0])


def test_device_csr_in_device_csr_out():
    X = planted_csr()
    data = DeviceCSR(X, "cpu", contextual=np.ones((70, 3), dtype=np.float32))
    kept, rest = thin.split(data, 0.5, seed=3)         # engine=None: host off-GPU
    ok, orr = oracle_split(X, 0.5, 3)
    for got, ref in ((kept, ok), (rest, orr)):
        assert isinstance(got, DeviceCSR) and (got.n_docs, got.vocab_size) == X.shape
        assert got.indptr.dtype == torch.int32 and got.values.dtype == torch.float32
        np.testing.assert_array_equal(got.indptr.numpy(), ref.indptr)
        np.testing.assert_array_equal(got.indices.numpy(), ref.indices)
        np.testing.assert_array_equal(got.values.numpy(), ref.data)
        assert got.nnz == ref.nnz and got.row_len_max == int(np.diff(ref.indptr).max())
        assert got.contextual is data.contextual        # shared, not copied
    with pytest.raises(RuntimeError):
        thin.split(data, 0.5, seed=3, engine="fused")   # the corpus is not on a GPU
    with pytest.raises(ValueError):
        thin.split(data, 0.5, seed=3, engine="numpy")


def test_rates_zero_and_one_and_seeds():
    X = planted_csr()
    kept, rest = thin.split(X, 0.0, seed=1, engine="host")
    assert kept.nnz == 0 and kept.shape == X.shape and len(kept.indptr) == 71
    assert_same_csr(rest, X)
    kept, rest = thin.split(X, 1.0, seed=1, engine="host")
    assert rest.nnz == 0 and rest.shape == X.shape
    assert_same_csr(kept, X)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            thin.split(X, bad, seed=1, engine="host")
    a, b = thin.split(X, 0.5, seed=1, engine="host")[0], thin.split(X, 0.5, seed=2, engine="host")[0]
    assert (a != b).nnz > 0
    assert_same_csr(a, thin.split(X, 0.5, seed=1, engine="host")[0])


def test_bad_counts_raise():
    X = planted_csr()
    for v in (1.5, -1.0, 65536.0, np.nan):
        Y = X.copy()
        Y.data[5] = v
        with pytest.raises(ValueError):
            thin.split(Y, 0.5, seed=0, engine="host")
    Y = X.copy()
    Y.data[5] = 65535.0                                 # the largest count allowed
    kept, rest = thin.split(Y, 0.5, seed=0, engine="host")
    assert (kept + rest != Y).nnz == 0


def test_kept_fraction():
    X = random_csr(400, 700, 40, seed=5)
    rate, N = 0.3, float(X.sum())
    kept, _ = thin.split(X, rate, seed=11, engine="host")
    assert N > 15000
    assert abs(kept.sum() / N - rate) <= 4 * np.sqrt(rate * (1 - rate) / N)


# ------------------------------------------------------------------------------ score
def _avitm(model_type, X, seed=0):
    torch.manual_seed(seed)
    tm = AVITM(input_size=X.shape[1], n_components=8, model_type=model_type, hidden_sizes=(16, 12),
               batch_size=32, lr=5e-3, verbose=False, device="cpu", backend="torch")
    ds = BOWDataset(X, VOCAB)
    for ep in range(2):                   # non-trivial running statistics
        tm._train_epoch(ds, seed=ep)
    return tm, ds


@pytest.mark.parametrize("model_type", ["prodLDA", "LDA"])
@pytest.mark.parametrize("S", [0, 2])
def test_completion_score_matches_formula(model_type, S):
    X = random_csr(70, 300, 30, seed=2)
    tm, ds = _avitm(model_type, X)
    n, K = X.shape[0], tm.n_components
    eps = np.random.default_rng(7).standard_normal((S, n, K)) if S else None
    got = tm.score(ds, n_samples=S, eps=eps, completion=0.5, split_seed=21)
    Xk, Xr = oracle_split(X, 0.5, 21)
    ref = oracle_completion(tm, Xk, Xr, eps)
    assert got["engine"] == "torch" and got["completion"] == 0.5
    assert got["tokens_observed"] == int(Xk.sum()) and got["tokens_heldout"] == int(Xr.sum())
    assert got["tokens_observed"] + got["tokens_heldout"] == int(X.sum())
    np.testing.assert_allclose(got["kl"], ref["kl"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(got["rl"], ref["rl"], rtol=1e-4, atol=1e-2)
    # predictive perplexity: the held-out reconstruction term alone, per held-out token
    assert got["perplexity"] == float(np.exp(got["rl"].astype(np.float64).sum() / got["tokens_heldout"]))
    np.testing.assert_allclose(got["perplexity"], np.exp(ref["rl"].sum() / Xr.sum()), rtol=1e-5)
    if S == 0:
        assert tm.perplexity(ds, n_samples=0, completion=0.5, split_seed=21) == got["perplexity"]
        # the default split seed is the scoring seed
        a = tm.score(ds, n_samples=0, seed=21, completion=0.5)
        np.testing.assert_array_equal(a["rl"], got["rl"])
        full = tm.score(ds, n_samples=0)                # completion=None: today's result
        assert "completion" not in full and not np.array_equal(full["rl"], got["rl"])
    assert tm.model.training


def test_score_rejects_degenerate_completion():
    X = random_csr(40, 300, 30, seed=2)
    tm, ds = _avitm("prodLDA", X)
    for bad in (0.0, 1.0, -0.5, 2):
        with pytest.raises(ValueError):
            tm.score(ds, n_samples=0, completion=bad)


# ------------------------------------------------------------------------------ HTM-WS
def test_htm_ws_counts_keyed():
    X = sp.csr_matrix(np.array([[2, 0, 3], [1, 4, 0]], dtype=np.float32))
    th = np.array([[1.0, 0.0], [0.0, 1.0]])
    be = np.full((2, 3), 1 / 3)
    out = htm_ws_counts(X, th, be, topic=0, seed=0, engine="keyed")
    assert np.array_equal(out.toarray(), [[2, 0, 3], [0, 0, 0]])
    # p = 1/2 everywhere: Binomial(40, 1/2) per non-zero
    X = sp.csr_matrix(np.full((200, 5), 40, dtype=np.float32))
    args = (X, np.full((200, 2), 0.5), np.full((2, 5), 0.2), 0)
    a = htm_ws_counts(*args, seed=1, engine="keyed")
    out = a.toarray()
    assert abs(out.mean() - 20) < 0.5 and out.max() <= 40
    assert_same_csr(a, htm_ws_counts(*args, seed=1, engine="keyed"))
    assert_same_csr(a, htm_ws_counts(*args, seed=1, engine="keyed", chunk=7))
    assert (a != htm_ws_counts(*args, seed=2, engine="keyed")).nnz > 0
    # the draws are the oracle's, at p = 1/2
    ref = oracle_kept(1, csr_rows(X), X.indices, X.data, np.full(X.nnz, 0.5))
    np.testing.assert_array_equal(out.ravel(), ref)
    with pytest.raises(ValueError):
        htm_ws_counts(*args, seed=1, engine="philox")


def test_responsibilities_host():
    X = planted_csr()
    rng = np.random.default_rng(0)
    K, e = 7, 3                                         # an odd K: the k-sum's tail term
    th = rng.dirichlet(np.full(K, 0.3), size=70)
    th[3] = 0.0
    th[5] = np.eye(K)[e]
    tw = rng.dirichlet(np.full(700, 0.05), size=K)
    kept, p = thin.thin_by_topic(X, th, tw, e, seed=4, engine="host", return_p=True)
    rows = csr_rows(X)
    den = (th[rows] * tw[:, X.indices].T).sum(1)
    ref = np.where(den > 0, th[rows, e] * tw[e, X.indices] / np.where(den > 0, den, 1), 0.0)
    np.testing.assert_allclose(p, ref, rtol=1e-4, atol=1e-7)
    assert_same_csr(kept, _part(X, oracle_kept(4, rows, X.indices, X.data, p)))
    assert kept[3].nnz == 0 and (kept[5] != X[5]).nnz == 0
    with pytest.raises(ValueError):
        thin.thin_by_topic(X, th, tw, K, seed=4, engine="host")


def test_wrapper_keyed_submodel_corpus_is_reproducible(tmp_path):
    from tests.test_tm_wrapper import _docs, _params
    pq = tmp_path / "corpus.parquet"
    pd.DataFrame({"id": range(60), "bow_text": _docs(60, 0)}).to_parquet(pq)
    w = TMWrapper(device="cpu", seed=3, htm_engine="keyed")
    root = w.train_root_model(str(tmp_path / "models"), "root", str(pq), "avitm", _params())
    a = w.create_submodel_corpus(root, "HTM-WS", 0)
    b = TMWrapper(device="cpu", seed=3, htm_engine="keyed").create_submodel_corpus(root, "HTM-WS", 0)
    assert 0 < len(a) <= 60
    pd.testing.assert_frame_equal(a, b)
    c = TMWrapper(device="cpu", seed=4, htm_engine="keyed").create_submodel_corpus(root, "HTM-WS", 0)
    assert not a["bow_text"].equals(c["bow_text"])
    with pytest.raises(ValueError):
        TMWrapper(device="cpu", htm_engine="fused")
