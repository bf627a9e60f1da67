"""The fused scorer on the NeuralLDA decoder and with a label head (csrc/score.hip
gfk_score_ext, FusedEngine.score, TopicModelBase.score(engine="fused")) against the float64
oracle of tests/score_oracle.py fed the kernel's own Philox draws, and the federated
document-completion perplexity on the GPU.

Tolerances are the project's per-row ones (tests/test_score_gpu.py); CE rows are held to the
KL tolerance.  Every comparison prints its worst error and the fraction of the tolerance it
uses (docs/PARITY.md section 4.2 quotes them).
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan, BOWDataset, CTMDataset, DeviceCSR
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from gfedntm_amd.ops import thin
from gfedntm_amd.ops.engine import score_covers, score_supports
from tests.helpers import random_csr, row_edge_csr
from tests.infer_oracle import np_state, perturb_state
from tests.score_oracle import oracle_loss, oracle_score
from tests.test_theta_infer import _trained, infer_normals
from tests.test_thin import oracle_completion, oracle_split

pytestmark = pytest.mark.gpu

VOCAB = {i: str(i) for i in range(8200)}
SEED = 0x5EED_1234
SPLIT_SEED = 0x51A7
KL_TOL = dict(rtol=1e-4, atol=1e-3)
RL_TOL = dict(rtol=1e-4, atol=1e-2)

_MODELS = {}


def _model(K, V):
    """A NeuralLDA model after a few fused steps, D = 300 documents; one per shape, shared."""
    if (K, V) not in _MODELS:
        _MODELS[K, V] = _trained(K=K, H=(32, 24), V=V, n_docs=300, model_type="LDA")
    return _MODELS[K, V]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _draws(n, K, S):
    return infer_normals(SEED, n, K, S) if S else None


def _used(got, ref, rtol, atol):
    """(largest |error|, largest fraction of the tolerance atol + rtol |ref| in use)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float(err.max()), float((err / (atol + rtol * np.abs(ref))).max())


def _assert_matches(got, ref, what=""):
    got = got.double().cpu().numpy()
    cols = [("kl", 0, KL_TOL), ("rl", 1, RL_TOL)] + ([("ce", 2, KL_TOL)] if got.shape[1] == 3 else [])
    for name, j, tol in cols:
        print(what, name, "max |err| %.3e, fraction of the tolerance %.3f" % _used(got[:, j], ref[name], **tol))
    assert np.isfinite(got).all()
    for name, j, tol in cols:
        np.testing.assert_allclose(got[:, j], ref[name], **tol)


def _vranges(tm):
    return int(tm.engine.lib.gfk_score_vranges(C.byref(tm.engine._m)))


# (20, 700): a tail of 60 columns; (200, 8200): beta's row stride padded to 8256 and two
# vocabulary ranges; (256, 700): four topics per lane in the theta kernel, the kernels' K limit
@pytest.mark.parametrize("K,V", [(20, 700), (50, 4466), (200, 8200), (256, 700)])
@pytest.mark.parametrize("S", [0, 1, 3])
def test_matches_oracle(K, V, S):
    tm, X, data = _model(K, V)
    assert not tm.model.is_prodlda and score_covers(tm) and not score_supports(tm)
    if V >= 8192:
        assert int(tm.engine._m.ldb) == 8256 and _vranges(tm) == 2
    got = tm.engine.score(data, n_samples=S, seed=SEED)
    assert got.shape == (300, 2)
    _assert_matches(got, oracle_score(tm, X, _draws(300, K, S)), f"K={K} V={V} S={S}")


def test_unbounded_logits():
    """Running statistics do not bound zn: beta scaled until every topic's largest zn exceeds
    100 (an unshifted fp32 exp overflows at 88.7 for every topic), some scored non-zero has
    p < 1e-10, where the +1e-10 decides the term, and others keep p far above it."""
    torch.manual_seed(0)
    K, V = 20, 701
    tm = AVITM(input_size=V, n_components=K, model_type="LDA", hidden_sizes=(32, 24), batch_size=64,
               verbose=False, device="cuda", backend="fused")
    perturb_state(tm, seed=3)
    with torch.no_grad():
        tm.model.beta.mul_(2500.0)
    torch.cuda.synchronize()
    X, _ = row_edge_csr(V, seed=1)
    data = DeviceCSR(X, "cuda")
    sd = np_state(tm)
    zn = (sd["beta"] - sd["beta_batchnorm.running_mean"]) / np.sqrt(
        sd["beta_batchnorm.running_var"] + tm.model.beta_batchnorm.eps)
    print("largest |zn|", np.abs(zn).max(), "smallest per-topic maximum", zn.max(1).min())
    assert zn.max(1).min() > 100.0
    for S in (0, 2):
        ref = oracle_score(tm, X, _draws(X.shape[0], K, S))
        print("S", S, "p_nz_min", ref["p_nz_min"], "p_nz_max", ref["p_nz_max"], "max RL", ref["rl"].max())
        assert ref["p_nz_min"] < 1e-10 and ref["p_nz_max"] > 1e-4 and np.isfinite(ref["rl"]).all()
        _assert_matches(tm.engine.score(data, n_samples=S, seed=SEED), ref, f"unbounded S={S}")


def test_edge_rows():
    """Empty first / middle / last documents, rows of 1, 63, 64, 65, 127, 128, 129 and 400
    non-zeros, single non-zeros at column 0 and V - 1, a count of 1000."""
    tm, _, _ = _model(20, 700)
    X, marks = row_edge_csr(700, seed=2)
    data = DeviceCSR(X, "cuda")
    for S in (0, 3):
        got = tm.engine.score(data, n_samples=S, seed=SEED)
        _assert_matches(got, oracle_score(tm, X, _draws(X.shape[0], 20, S)), f"edge S={S}")
        for name in ("empty_first", "empty_mid", "empty_last"):
            assert float(got[marks[name], 1]) == 0.0


def test_chunk_and_grid_independence():
    tm, _, data = _model(50, 4466)
    a = tm.engine.score(data, n_samples=3, seed=5)
    assert torch.equal(a, tm.engine.score(data, n_samples=3, seed=5, chunk=37))    # 9 launches, doc0 != 0
    assert not torch.equal(a[:, 1], tm.engine.score(data, n_samples=3, seed=6)[:, 1])
    kept, rest = thin.split(data, 0.5, SEED)
    for S in (1, 3):                                        # both instances of the sparse kernel
        b = tm.engine.score(kept, n_samples=S, seed=5, target=rest)
        for g in (1, 3):
            # a wave takes several documents, a workgroup several (topic, range) items
            assert 300 > 4 * g and 50 * _vranges(tm) > g
            assert torch.equal(b, tm.engine.score(kept, n_samples=S, seed=5, target=rest, max_grid=g))
        assert not torch.equal(a[:, 1], b[:, 1])
    # two vocabulary ranges: the ranges' merge on fewer workgroups than items
    tm2, _, data2 = _model(200, 8200)
    assert _vranges(tm2) == 2
    assert torch.equal(tm2.engine.score(data2, n_samples=1, seed=5),
                       tm2.engine.score(data2, n_samples=1, seed=5, max_grid=3, chunk=101))


@pytest.mark.parametrize("S", [0, 3])
def test_document_completion(S):
    tm, X, _ = _model(20, 700)
    ds = BOWDataset(X, VOCAB)
    Xk, Xr = oracle_split(X, 0.5, SPLIT_SEED)
    ref = oracle_completion(tm, Xk, Xr, _draws(300, 20, S))
    r = tm.score(ds, n_samples=S, seed=SEED, engine="fused", completion=0.5, split_seed=SPLIT_SEED)
    assert r["engine"] == "fused" and r["completion"] == 0.5 and "ce" not in r
    assert r["tokens_observed"] == int(Xk.sum()) and r["tokens_heldout"] == int(Xr.sum())
    print("completion S", S, "kl", _used(r["kl"], ref["kl"], **KL_TOL), "rl", _used(r["rl"], ref["rl"], **RL_TOL))
    np.testing.assert_allclose(r["kl"], ref["kl"], **KL_TOL)
    np.testing.assert_allclose(r["rl"], ref["rl"], **RL_TOL)
    assert r["perplexity"] == float(np.exp(r["rl"].astype(np.float64).sum() / r["tokens_heldout"]))
    assert tm.perplexity(ds, n_samples=S, seed=SEED, completion=0.5, split_seed=SPLIT_SEED,
                         engine="fused") == r["perplexity"]
    # the default does not move
    assert tm.score(ds, n_samples=1, seed=SEED)["engine"] == "torch"


def _label_kw(model_type):
    return dict(input_size=700, contextual_size=32, n_components=20, hidden_sizes=(32, 32), batch_size=64,
                verbose=False, device="cuda", label_size=5, model_type=model_type)


@pytest.mark.parametrize("cls,model_type", [(CombinedTM, "prodLDA"), (ZeroShotTM, "prodLDA"),
                                            (CombinedTM, "LDA")])
def test_label_head(cls, model_type):
    torch.manual_seed(0)
    V, C_, K, n, S, L = 700, 32, 20, 150, 2, 5
    kw = _label_kw(model_type)
    X = random_csr(n, V, 30, seed=3)
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((n, C_)).astype(np.float32)
    lab = np.eye(L, dtype=np.float32)[rng.integers(0, L, n)]
    tm = cls(backend="fused", **kw)           # (supports() accepts a CTM with model_type="LDA")
    ds = CTMDataset(emb, X, VOCAB, labels=lab)
    data = tm.device_data(ds)
    tm.engine.bind_data(data, BatchPlan.build(n, 64, 3, seed=0))
    for s in range(3):
        tm.engine.step(s)
    torch.cuda.synchronize()
    assert score_covers(tm) and not score_supports(tm)
    eps = infer_normals(SEED, n, K, S)
    ref = oracle_score(tm, X, eps, emb, lab)
    got = tm.engine.score(data, n_samples=S, seed=SEED)
    assert got.shape == (n, 3)
    _assert_matches(got, ref, f"{cls.__name__} {model_type}")
    assert torch.equal(got, tm.engine.score(data, n_samples=S, seed=SEED, chunk=37, max_grid=2))

    r = tm.score(ds, n_samples=S, seed=SEED, engine="fused")
    assert r["engine"] == "fused"
    np.testing.assert_array_equal(np.stack([r["kl"], r["rl"], r["ce"]], 1), got.cpu().numpy())
    kl_weight = float(tm.weights.get("beta", 1))
    assert [len(r["ce"][a:a + 64]) for a in range(0, n, 64)] == [64, 64, 22]
    np.testing.assert_allclose(r["loss"], oracle_loss(ref["kl"], ref["rl"], kl_weight, ref["ce"], 64), rtol=1e-4)
    assert tm.score(ds, n_samples=S, seed=SEED)["engine"] == "torch"       # the default does not move

    ref_tm = cls(backend="torch", **kw)
    ref_tm.model.load_state_dict({k: v.detach().clone() for k, v in tm.model.state_dict().items()})
    t = ref_tm.score(ds, n_samples=S, eps=eps)
    assert t["engine"] == "torch"
    np.testing.assert_allclose(r["kl"], t["kl"], **KL_TOL)
    np.testing.assert_allclose(r["rl"], t["rl"], **RL_TOL)
    np.testing.assert_allclose(r["ce"], t["ce"], **KL_TOL)
    np.testing.assert_allclose(r["loss"], t["loss"], rtol=1e-4)

    with pytest.raises(ValueError):
        tm.engine.score(DeviceCSR(X, "cuda", emb), n_samples=S, seed=SEED)
    with pytest.raises(ValueError):
        tm.score(CTMDataset(emb, X, VOCAB), n_samples=S, seed=SEED, engine="fused")


def test_label_argmax_takes_the_lowest_index():
    """Label rows with ties (two equal maxima, an all-zero row): the target is the first."""
    torch.manual_seed(0)
    n, L = 70, 5
    kw = _label_kw("prodLDA")
    X = random_csr(n, 700, 30, seed=4)
    rng = np.random.default_rng(1)
    emb = rng.standard_normal((n, 32)).astype(np.float32)
    lab = np.eye(L, dtype=np.float32)[rng.integers(0, L, n)]
    lab[3] = [0, 1, 0, 1, 0]
    lab[4] = 0
    lab[5] = [0.5, 2, 2, 2, 0.5]
    tm = perturb_state(CombinedTM(backend="fused", **kw), seed=5)
    torch.cuda.synchronize()
    ref = oracle_score(tm, X, None, emb, lab)
    got = tm.engine.score(DeviceCSR(X, "cuda", emb, lab), n_samples=0, seed=SEED)
    _assert_matches(got, ref, "label ties")


def test_federation_perplexity():
    from gfedntm_amd.data.synthetic import generate_synthetic
    from gfedntm_amd.federation.data import ClientCorpus
    from gfedntm_amd.federation.runner import LocalFederation
    from gfedntm_amd.utils.config import load_config
    sc = generate_synthetic(vocab_size=500, n_topics=5, n_docs=60, n_nodes=3, frozen_topics=2,
                            nwords=(20, 40), seed=1)
    params = dict(load_config().training_params)
    params.update(num_epochs=2, batch_size=32, hidden_sizes=(32, 24), n_components=10, model_type="LDA")
    fed = LocalFederation([ClientCorpus(synthetic=sc, node=i) for i in range(3)], params, max_iters=4,
                          device="cuda", backend="fused", seed=2)
    fed.run()
    torch.cuda.synchronize()
    tm = fed.clients[0].tm
    assert tm.backend == "fused" and not tm.model.is_prodlda
    seed, S = 11, 2
    got = fed.perplexity(completion=0.5, n_samples=S, seed=seed)
    assert got["engine"] == "fused" and got["clients"] == 3 and got["completion"] == 0.5
    assert got["n_docs"] == sum(c.n_docs for c in fed.clients)
    # the token counts: host splits with seeds seed + c, document indices local
    held = obs = 0
    rl_torch, n_docs = 0.0, 0
    for c in fed.clients:
        hk, hr = thin.split(c.dataset.csr, 0.5, seed + c.id, engine="host")
        obs, held = obs + int(hk.sum()), held + int(hr.sum())
        # the torch path on the same split, fed the kernel's normals
        eps = infer_normals(seed + c.id, c.n_docs, tm.n_components, S)
        t = tm.score(c.dataset, n_samples=S, eps=eps, completion=0.5, split_seed=seed + c.id)
        assert t["engine"] == "torch" and t["tokens_heldout"] == int(hr.sum())
        rl_torch += float(t["rl"].astype(np.float64).sum())
        n_docs += c.n_docs
    assert (got["tokens_observed"], got["tokens_heldout"]) == (obs, held)
    tol = RL_TOL["atol"] * n_docs + RL_TOL["rtol"] * abs(rl_torch)
    print("federation rl_sum", got["rl_sum"], "torch", rl_torch, "fraction of the tolerance",
          abs(got["rl_sum"] - rl_torch) / tol)
    assert abs(got["rl_sum"] - rl_torch) <= tol
    assert got["perplexity"] == float(np.exp(got["rl_sum"] / held))
    t = fed.perplexity(completion=0.5, n_samples=S, seed=seed, engine="torch")
    assert t["engine"] == "torch" and t["tokens_heldout"] == held and np.isfinite(t["perplexity"])
