"""Held-out scoring kernels (csrc/score.hip, FusedEngine.score) against the float64 oracle
written out from the model's state_dict, fed the kernel's own Philox draws."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BatchPlan, BOWDataset, CTMDataset, DeviceCSR
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from tests.helpers import random_csr
from tests.score_oracle import oracle_score
from tests.test_theta_infer import _trained, infer_normals

pytestmark = pytest.mark.gpu

VOCAB = {i: str(i) for i in range(8200)}
SEED = 0x5EED_1234
# the project's per-row loss tolerances (tests/test_fused_kernels.py)
KL_TOL = dict(rtol=1e-4, atol=1e-3)
RL_TOL = dict(rtol=1e-4, atol=1e-2)


_MODELS = {}


def _model(K, V):
    """A model after a few fused steps (non-trivial running statistics), D = 300 documents:
    the row blocks of 64 / 32 rows have a tail.  Trained once per shape and shared."""
    if (K, V) not in _MODELS:
        _MODELS[K, V] = _trained(K=K, H=(32, 24), V=V, n_docs=300)
    return _MODELS[K, V]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The shared models leave with the module: later tests find the allocator empty."""
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _draws(n, K, S):
    return infer_normals(SEED, n, K, S) if S else None


def _assert_matches(got, ref):
    got = got.double().cpu().numpy()
    print("max |dKL|", np.abs(got[:, 0] - ref["kl"]).max(), "max |dRL|", np.abs(got[:, 1] - ref["rl"]).max(),
          "max rel dRL", (np.abs(got[:, 1] - ref["rl"]) / np.maximum(np.abs(ref["rl"]), 1e-30)).max())
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got[:, 0], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(got[:, 1], ref["rl"], **RL_TOL)


# (20, 700): a tail tile of 60 columns; (200, 8200): beta's row stride padded to 8256 and a
# tail tile; (300, 700): several k-chunks, 32-row blocks
@pytest.mark.parametrize("K,V", [(20, 700), (50, 4466), (200, 8200), (300, 700)])
@pytest.mark.parametrize("S", [0, 1, 3])
def test_score_matches_oracle(K, V, S):
    tm, X, data = _model(K, V)
    if V >= 8192:
        assert int(tm.engine._m.ldb) == 8256
    got = tm.engine.score(data, n_samples=S, seed=SEED)
    _assert_matches(got, oracle_score(tm, X, _draws(X.shape[0], K, S)))


def test_unbounded_logits():
    """Running statistics do not bound the logits: beta scaled until the oracle's largest
    |zn| exceeds 100 (exp overflows fp32 at 88.7) and some scored non-zero has
    p < 1e-10, where the +1e-10 decides the term -- while other non-zeros keep a p far
    above it, so a wrong log-sum-exp cannot hide behind the floor."""
    tm, X, data = _trained(K=20, H=(32, 24), V=700, n_docs=300)
    with torch.no_grad():
        tm.model.beta.mul_(2500.0)
    torch.cuda.synchronize()
    for S in (0, 2):
        ref = oracle_score(tm, X, _draws(X.shape[0], 20, S))
        print("zn_absmax", ref["zn_absmax"], "p_nz_min", ref["p_nz_min"], "p_nz_max", ref["p_nz_max"])
        assert ref["zn_absmax"] > 100.0 and ref["p_nz_min"] < 1e-10     # not vacuous
        assert ref["p_nz_max"] > 1e-4
        _assert_matches(tm.engine.score(data, n_samples=S, seed=SEED), ref)


def test_edge_rows():
    """No non-zeros; every non-zero in the last, partial tile; 400 non-zeros."""
    tm, _, _ = _model(20, 700)
    V = 700
    X = random_csr(70, V, 40, seed=9).tolil()
    rng = np.random.default_rng(3)
    X[0, :] = 0
    X[1, :] = 0
    X[1, 640:700] = rng.integers(0, 3, 60)
    X[1, 699] = 2
    X[2, :] = 0
    X[2, rng.choice(V, 400, replace=False)] = rng.integers(1, 5, 400)
    X[69, :] = 0                                            # the last row, empty too
    X = sp.csr_matrix(X, dtype=np.float32)
    X.eliminate_zeros()
    X.sort_indices()
    assert X[0].nnz == 0 and X[1].indices.min() >= 640 and X[2].nnz == 400
    data = DeviceCSR(X, "cuda")
    for S in (0, 3):
        got = tm.engine.score(data, n_samples=S, seed=SEED)
        _assert_matches(got, oracle_score(tm, X, _draws(70, 20, S)))
        assert float(got[0, 1]) == 0.0 and float(got[69, 1]) == 0.0


def test_chunk_and_grid_independence():
    """Chunking and seed; the strided loops on fewer workgroups than work items are
    tests/test_eval_grid_gpu.py's."""
    tm, _, data = _model(50, 4466)
    a = tm.engine.score(data, n_samples=3, seed=5)
    # 9 launches, doc0 != 0; each launch's grid still covers its chunk in one pass
    assert torch.equal(a, tm.engine.score(data, n_samples=3, seed=5, chunk=37))
    assert torch.equal(a, tm.engine.score(data, n_samples=3, seed=5))
    assert not torch.equal(a[:, 1], tm.engine.score(data, n_samples=3, seed=6)[:, 1])


@pytest.mark.parametrize("cls", [CombinedTM, ZeroShotTM])
def test_ctm_matches_torch_engine(cls):
    torch.manual_seed(0)
    V, C, K, n, S = 700, 32, 20, 150, 2
    X = random_csr(n, V, 30, seed=3)
    emb = np.random.default_rng(0).standard_normal((n, C)).astype(np.float32)
    kw = dict(input_size=V, contextual_size=C, n_components=K, hidden_sizes=(32, 32),
              batch_size=64, verbose=False, device="cuda")
    tm = cls(backend="fused", **kw)
    ds = CTMDataset(emb, X, VOCAB)
    data = tm.device_data(ds)
    tm.engine.bind_data(data, BatchPlan.build(n, 64, 3, seed=0))
    for s in range(3):
        tm.engine.step(s)
    torch.cuda.synchronize()
    got = tm.score(ds, n_samples=S, seed=SEED)
    assert got["engine"] == "fused"
    ref_tm = cls(backend="torch", **kw)
    ref_tm.model.load_state_dict({k: v.detach().clone() for k, v in tm.model.state_dict().items()})
    ref = ref_tm.score(ds, n_samples=S, eps=infer_normals(SEED, n, K, S))
    assert ref["engine"] == "torch"
    np.testing.assert_allclose(got["kl"], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(got["rl"], ref["rl"], **RL_TOL)
    np.testing.assert_allclose(got["loss"], ref["loss"], rtol=1e-4)
    np.testing.assert_allclose(got["perplexity"], ref["perplexity"], rtol=1e-4)


def test_api_engines_and_validation():
    tm, X, _ = _model(20, 700)
    ds = BOWDataset(X, VOCAB)
    r = tm.score(ds, n_samples=1, seed=7)
    assert r["engine"] == "fused" and tm.engine_info["score_engine"] == "fused"
    np.testing.assert_array_equal(
        np.stack([r["kl"], r["rl"]], 1), tm.engine.score(tm.device_data(ds), 1, seed=7).cpu().numpy())
    assert tm._validate_epoch(ds, seed=7) == (X.shape[0], r["loss"])
    assert tm.perplexity(ds, seed=7) == r["perplexity"]

    lda, Xl, _ = _trained(K=20, H=(32, 24), V=700, n_docs=100, model_type="LDA")
    dl = BOWDataset(Xl, VOCAB)
    rl = lda.score(dl, n_samples=1, seed=7)
    assert rl["engine"] == "torch" and np.isfinite(rl["loss"])
    info = lda.engine_info
    assert info["engine"] == "fused" and info["score_engine"] == "torch"
    assert "NeuralLDA" in info["score_fused_unavailable"]


def test_fit_with_validation_on_the_fused_backend():
    torch.manual_seed(0)
    X, Xv = random_csr(128, 700, 40, seed=1), random_csr(64, 700, 40, seed=2)
    tm = AVITM(input_size=700, n_components=20, hidden_sizes=(32, 24), batch_size=64, num_epochs=2,
               verbose=False, device="cuda", backend="fused")
    seen = []
    inner = tm._validate_epoch
    tm._validate_epoch = lambda ds, *a, **k: (seen.append(inner(ds, *a, **k)) or seen[-1])
    tm.fit(BOWDataset(X, VOCAB), BOWDataset(Xv, VOCAB), n_samples=2)
    assert tm.nn_epoch == 1 and len(seen) == 2
    assert all(n == 64 and np.isfinite(v) for n, v in seen)
