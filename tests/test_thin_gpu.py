"""Thinning kernels (csrc/thin.hip, gfedntm_amd/ops/thin.py) against the float64 oracle of
the keyed draws, and document-completion scoring on the fused engine against the float64
formula on the oracle's own split."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BatchPlan, BOWDataset, CTMDataset, DeviceCSR
from gfedntm_amd.models import CombinedTM
from gfedntm_amd.ops import thin
from tests.helpers import random_csr
from tests.test_score_gpu import KL_TOL, RL_TOL
from tests.test_theta_infer import _trained, infer_normals
from tests.test_thin import (_part, assert_same_csr, csr_rows, oracle_completion, oracle_kept,
                             oracle_split, planted_csr)

pytestmark = pytest.mark.gpu

VOCAB = {i: str(i) for i in range(8200)}
SEED = 0x5EED_1234
SPLIT_SEED = (9 << 32) | 77


def _host(d: DeviceCSR) -> sp.csr_matrix:
    return sp.csr_matrix((d.values.cpu().numpy(), d.indices.cpu().numpy(), d.indptr.cpu().numpy()),
                         shape=(d.n_docs, d.vocab_size))


def _same_device_csr(a: DeviceCSR, b: DeviceCSR):
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
    assert torch.equal(a.values, b.values)


# ------------------------------------------------------------------------------ split
@pytest.mark.parametrize("rate", [0.3, 0.5])
def test_split_equals_oracle(rate):
    X = planted_csr()
    data = DeviceCSR(X, "cuda")
    kept, rest = thin.split(data, rate, SPLIT_SEED)              # engine=None: the kernels
    ok, orr = oracle_split(X, rate, SPLIT_SEED)
    for got, ref in ((kept, ok), (rest, orr)):
        assert isinstance(got, DeviceCSR) and got.device.type == "cuda"
        g = _host(got)
        assert (g.data > 0).all()                                # no zero is stored
        for d in range(70):                                      # rows stay sorted
            assert (np.diff(g.indices[g.indptr[d]:g.indptr[d + 1]]) > 0).all()
        assert_same_csr(g, ref)
        assert got.nnz == ref.nnz and got.row_len_max == int(np.diff(ref.indptr).max())
    assert (_host(kept) + _host(rest) != X).nnz == 0
    hk, hr = thin.split(X, rate, SPLIT_SEED, engine="host")       # fused == host, exactly
    assert_same_csr(_host(kept), hk)
    assert_same_csr(_host(rest), hr)
    # chunk=37: two launches, doc0 = 37 (grids smaller than the work: tests/test_eval_grid_gpu.py)
    for other in (thin.split(data, rate, SPLIT_SEED, chunk=37),
                  thin.split(X, rate, SPLIT_SEED, engine="fused")):
        _same_device_csr(other[0], kept)
        _same_device_csr(other[1], rest)
    assert not torch.equal(thin.split(data, rate, SPLIT_SEED + 1)[0].values, kept.values)


def test_split_extremes_and_bad_counts():
    X = planted_csr()
    data = DeviceCSR(X, "cuda", contextual=np.ones((70, 3), dtype=np.float32))
    kept, rest = thin.split(data, 0.0, 1)
    assert kept.nnz == 0 and int(kept.indptr.abs().sum()) == 0 and kept.indptr.numel() == 71
    assert_same_csr(_host(rest), X)
    assert rest.contextual is data.contextual                    # shared, not copied
    kept, rest = thin.split(data, 1.0, 1)
    assert rest.nnz == 0 and rest.row_len_max == 0
    assert_same_csr(_host(kept), X)
    for v in (1.5, -1.0, 65536.0):
        Y = X.copy()
        Y.data[5] = v
        with pytest.raises(ValueError):
            thin.split(DeviceCSR(Y, "cuda"), 0.5, 0)


# ------------------------------------------------------------------------------ responsibilities
@pytest.mark.parametrize("K", [20, 50, 200])
@pytest.mark.parametrize("V,ld", [(700, 700), (8200, 8256)])
def test_responsibilities(K, V, ld):
    X = planted_csr(V)
    rng = np.random.default_rng(K + V)
    e = K // 3
    th = rng.dirichlet(np.full(K, 0.3), size=70).astype(np.float32)
    th[3] = 0.0                                                  # p = 0: keeps nothing
    th[5] = np.eye(K, dtype=np.float32)[e]                       # p = 1: keeps everything
    # rows of a softmax over the vocabulary, spread over ~5 decades (no fp32 underflow in
    # theta x tw: the float64 oracle would not see it)
    z = rng.standard_normal((K, V)) * 2.5
    tw = (np.exp(z) / np.exp(z).sum(1, keepdims=True)).astype(np.float32)
    wide = torch.zeros(K, ld, device="cuda")
    wide[:, :V] = torch.from_numpy(tw).cuda()
    data = DeviceCSR(X, "cuda")
    kept, p = thin.thin_by_topic(data, th, wide[:, :V], e, SEED, return_p=True)
    assert isinstance(kept, DeviceCSR) and p.shape == (X.nnz,) and p.dtype == torch.float32
    rows = csr_rows(X)
    t64, w64 = th.astype(np.float64), tw.astype(np.float64)
    den = (t64[rows] * w64[:, X.indices].T).sum(1)
    ref = np.where(den > 0, t64[rows, e] * w64[e, X.indices] / np.where(den > 0, den, 1), 0.0)
    pk = p.cpu().numpy()
    print("max |dp|", np.abs(pk - ref).max(), "max rel", (np.abs(pk - ref) / np.maximum(ref, 1e-30)).max())
    np.testing.assert_allclose(pk, ref, rtol=1e-4, atol=1e-7)
    assert (pk >= 0).all() and (pk <= 1).all()
    # the kept counts are the keyed draws at the kernel's own p: every non-zero
    assert_same_csr(_host(kept), _part(X, oracle_kept(SEED, rows, X.indices, X.data, pk)))
    assert (pk[rows == 3] == 0).all() and _host(kept)[3].nnz == 0
    assert (pk[rows == 5] == 1).all() and (_host(kept)[5] != X[5]).nnz == 0
    assert 0 < kept.nnz < X.nnz
    # chunking and a second run: bitwise
    again, p2 = thin.thin_by_topic(data, th, wide[:, :V], e, SEED, return_p=True, chunk=37)
    _same_device_csr(again, kept)
    assert torch.equal(p, p2)
    # the host twin's p agrees to fp32 rounding
    _, ph = thin.thin_by_topic(X, th, tw, e, SEED, engine="host", return_p=True)
    np.testing.assert_allclose(pk, ph, rtol=1e-4, atol=1e-7)


def test_htm_ws_counts_keyed_on_gpu():
    from gfedntm_amd.experiments.tm_wrapper import htm_ws_counts
    X = sp.csr_matrix(np.array([[2, 0, 3], [1, 4, 0]], dtype=np.float32))
    out = htm_ws_counts(X, np.array([[1.0, 0.0], [0.0, 1.0]]), np.full((2, 3), 1 / 3), topic=0, seed=0,
                        device="cuda", engine="keyed")
    assert np.array_equal(out.toarray(), [[2, 0, 3], [0, 0, 0]])
    X = sp.csr_matrix(np.full((200, 5), 40, dtype=np.float32))
    args = (X, np.full((200, 2), 0.5), np.full((2, 5), 0.2), 0)
    a = htm_ws_counts(*args, seed=1, device="cuda", engine="keyed")
    assert abs(a.toarray().mean() - 20) < 0.5 and a.max() <= 40
    # p = 1/2 is exact on both engines: the GPU's corpus is the CPU's
    assert_same_csr(a, htm_ws_counts(*args, seed=1, device="cpu", engine="keyed"))


# ------------------------------------------------------------------------------ completion score
_MODELS = {}


def _model(K, V):
    if (K, V) not in _MODELS:
        _MODELS[K, V] = _trained(K=K, H=(32, 24), V=V, n_docs=300)
    return _MODELS[K, V]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("K,V", [(20, 700), (50, 4466)])
@pytest.mark.parametrize("S", [0, 3])
def test_completion_score_matches_oracle(K, V, S):
    tm, X, data = _model(K, V)
    Xk, Xr = oracle_split(X, 0.5, SPLIT_SEED)
    ref = oracle_completion(tm, Xk, Xr, infer_normals(SEED, X.shape[0], K, S) if S else None)
    kept, rest = thin.split(data, 0.5, SPLIT_SEED)
    got = tm.engine.score(kept, n_samples=S, seed=SEED, target=rest)
    g = got.double().cpu().numpy()
    print("max |dKL|", np.abs(g[:, 0] - ref["kl"]).max(), "max |dRL|", np.abs(g[:, 1] - ref["rl"]).max())
    assert np.isfinite(g).all()
    np.testing.assert_allclose(g[:, 0], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(g[:, 1], ref["rl"], **RL_TOL)
    # the device split is the oracle's: the same bits as scoring the host-built parts
    assert torch.equal(got, tm.engine.score(DeviceCSR(Xk, "cuda"), n_samples=S, seed=SEED,
                                            target=DeviceCSR(Xr, "cuda")))
    # ... and the public entry point runs exactly this
    r = tm.score(BOWDataset(X, VOCAB), n_samples=S, seed=SEED, completion=0.5, split_seed=SPLIT_SEED)
    assert r["engine"] == "fused" and r["completion"] == 0.5
    np.testing.assert_array_equal(np.stack([r["kl"], r["rl"]], 1), got.cpu().numpy())
    assert r["tokens_observed"] == int(Xk.sum()) and r["tokens_heldout"] == int(Xr.sum())
    assert r["perplexity"] == float(np.exp(r["rl"].astype(np.float64).sum() / r["tokens_heldout"]))
    assert not torch.equal(got[:, 1], tm.engine.score(data, n_samples=S, seed=SEED)[:, 1])


def test_completion_target_checks():
    tm, X, data = _model(20, 700)
    with pytest.raises(ValueError):
        tm.engine.score(data, target=DeviceCSR(X[:100], "cuda"))
    with pytest.raises(ValueError):
        tm.score(BOWDataset(X, VOCAB), completion=1.0)


def test_completion_combined_matches_torch_engine():
    torch.manual_seed(0)
    V, C, K, n, S = 700, 32, 20, 150, 2
    X = random_csr(n, V, 30, seed=3)
    emb = np.random.default_rng(0).standard_normal((n, C)).astype(np.float32)
    kw = dict(input_size=V, contextual_size=C, n_components=K, hidden_sizes=(32, 32),
              batch_size=64, verbose=False, device="cuda")
    tm = CombinedTM(backend="fused", **kw)
    ds = CTMDataset(emb, X, VOCAB)
    data = tm.device_data(ds)
    tm.engine.bind_data(data, BatchPlan.build(n, 64, 3, seed=0))
    for s in range(3):
        tm.engine.step(s)
    torch.cuda.synchronize()
    got = tm.score(ds, n_samples=S, seed=SEED, completion=0.5, split_seed=SPLIT_SEED)
    assert got["engine"] == "fused"
    ref_tm = CombinedTM(backend="torch", **kw)
    ref_tm.model.load_state_dict({k: v.detach().clone() for k, v in tm.model.state_dict().items()})
    ref = ref_tm.score(ds, n_samples=S, eps=infer_normals(SEED, n, K, S), completion=0.5,
                       split_seed=SPLIT_SEED)
    assert ref["engine"] == "torch"
    Xk, Xr = oracle_split(X, 0.5, SPLIT_SEED)
    for r in (got, ref):                                         # both engines: the oracle's split
        assert r["tokens_observed"] == int(Xk.sum()) and r["tokens_heldout"] == int(Xr.sum())
    np.testing.assert_allclose(got["kl"], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(got["rl"], ref["rl"], **RL_TOL)
    np.testing.assert_allclose(got["perplexity"], ref["perplexity"], rtol=1e-4)


def test_completion_neural_lda_runs_on_torch_with_the_same_split():
    lda, X, _ = _trained(K=20, H=(32, 24), V=700, n_docs=100, model_type="LDA")
    n, S = X.shape[0], 2
    eps = infer_normals(SEED, n, 20, S)
    r = lda.score(BOWDataset(X, VOCAB), n_samples=S, eps=eps, completion=0.5, split_seed=SPLIT_SEED)
    assert r["engine"] == "torch"
    Xk, Xr = oracle_split(X, 0.5, SPLIT_SEED)
    assert r["tokens_observed"] == int(Xk.sum()) and r["tokens_heldout"] == int(Xr.sum())
    ref = oracle_completion(lda, Xk, Xr, eps)
    np.testing.assert_allclose(r["kl"], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(r["rl"], ref["rl"], **RL_TOL)
    r2 = lda.score(BOWDataset(X, VOCAB), n_samples=1, seed=7, completion=0.5, split_seed=SPLIT_SEED)
    assert r2["engine"] == "torch" and np.isfinite(r2["loss"])
