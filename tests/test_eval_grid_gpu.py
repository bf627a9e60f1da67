"""The evaluation kernels' strided loops iterate more than once: every launch of theta
inference, held-out scoring, thinning and the co-occurrence pack on ``max_grid`` = 1 and 3
workgroups must give the bits of the default launch.

The default grids always cover their work in one pass (a wave or workgroup per work item up
to thousands of items), so no other test runs a second iteration of

* gfk_theta_infer_k's document loop (``abuf`` reused per wave, staged and unstaged weights),
* gfk_score_theta_k, gfk_doc_score_k (``th`` / ``part`` and the closing barrier, the online
  (max, sum) pairs and the prefetch registers re-initialised per work item), gfk_score_sparse_k
  (``trow``),
* gfk_thin_count_k / gfk_thin_compact_k (``trow``, the row's output slots),
* gfk_cooc_pack_k (the LDS masks cleared per group of 64 documents).

With a cap of 1 every wave walks about 20 to 40 work items of tests/helpers.row_edge_csr
(empty rows, rows of 63 ... 129 and 400 non-zeros, a count of 1000).  The default launches are
checked against float64 oracles elsewhere (tests/test_infer_walk_gpu.py, test_score_gpu.py,
test_thin_gpu.py, test_cooc_gpu.py): bitwise equality carries those checks to the looped runs.
gfk_score_mean_k (a thread per document, no loop) and gfk_cooc_count_k (integer atomics over
a grid that is a function of the shape) keep their grids.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import DeviceCSR
from gfedntm_amd.eval.metrics import cooccurrence_counts
from gfedntm_amd.models import AVITM
from gfedntm_amd.ops import thin
from tests.helpers import random_csr, row_edge_csr
from tests.infer_oracle import perturb_state

pytestmark = pytest.mark.gpu

GRIDS = (1, 3)
SEED = 0x5EED_1234
_MODELS = {}
_CORPORA = {}


def _corpus(V):
    if V not in _CORPORA:
        X, marks = row_edge_csr(V, seed=1)
        _CORPORA[V] = (X, DeviceCSR(X, "cuda"), marks)
    return _CORPORA[V]


def _model(K, V, H=(32, 24)):
    """An untrained fused ProdLDA model with a perturbed state (running statistics, weights),
    shared by the module."""
    if (K, V, H) not in _MODELS:
        torch.manual_seed(0)
        tm = AVITM(input_size=V, n_components=K, model_type="prodLDA", hidden_sizes=H, batch_size=16,
                   verbose=False, device="cuda", backend="fused")
        assert tm.backend == "fused"
        perturb_state(tm, seed=3)
        torch.cuda.synchronize()
        _MODELS[K, V, H] = tm
    return _MODELS[K, V, H]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _MODELS.clear()
    _CORPORA.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _same_csr(a: DeviceCSR, b: DeviceCSR):
    assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices)
    assert torch.equal(a.values, b.values)


# ------------------------------------------------------------------ theta inference
@pytest.mark.parametrize("H,K,staged", [((32, 24), 20, True), ((200, 200), 50, False)])
@pytest.mark.parametrize("mode", ["moments", "samples", "postprocess"])
def test_theta_infer(H, K, staged, mode):
    tm = _model(K, 701, H)
    e = tm.engine
    assert (int(e.lib.gfk_theta_infer_smem(C.byref(e._m))) <= 160 * 1024) == staged
    _, data, _ = _corpus(701)
    kw = {"moments": dict(moments=True), "samples": dict(n_samples=5, seed=SEED),
          "postprocess": dict(n_samples=5, seed=SEED, postprocess=True,
                              threshold=float(np.float32(3e-3)))}[mode]
    base = e.theta_infer(data, **kw)
    assert torch.isfinite(base).all() and -(-data.n_docs // 8) > max(GRIDS)
    if mode == "postprocess":
        assert (base == 0).any()
    for g in GRIDS:
        assert torch.equal(base, e.theta_infer(data, max_grid=g, **kw)), g
    with pytest.raises(ValueError):
        e.theta_infer(data, max_grid=0, **kw)


# ------------------------------------------------------------------ held-out scoring
# (20, 700): 64-row blocks (RT = 4), one vocabulary range; (200, 8200): two ranges, beta's
# row stride 8256, 7 k-chunks; (300, 700): 32-row blocks (RT = 2), 10 k-chunks
@pytest.mark.parametrize("K,V", [(20, 700), (200, 8200), (300, 700)])
@pytest.mark.parametrize("S", [0, 3])
def test_score(K, V, S):
    tm = _model(K, V)
    e = tm.engine
    _, data, _ = _corpus(V)
    if V >= 8192:
        assert int(e._m.ldb) == 8256 and int(e.lib.gfk_score_vranges(C.byref(e._m))) == 2
    target = thin.split(data, 0.5, SEED)[1]      # the sparse term reads another CSR than the encoder
    assert int(target.indices.numel()) not in (0, int(data.indices.numel()))
    base = e.score(data, n_samples=S, seed=SEED, target=target)
    assert torch.isfinite(base).all()
    rows = data.n_docs * max(S, 1)
    assert -(-rows // (64 if K <= 256 else 32)) > min(GRIDS)       # several row blocks per workgroup
    for g in GRIDS:
        assert torch.equal(base, e.score(data, n_samples=S, seed=SEED, target=target, max_grid=g)), g
    assert torch.equal(e.score(data, n_samples=S, seed=SEED),
                       e.score(data, n_samples=S, seed=SEED, max_grid=1))
    with pytest.raises(ValueError):
        e.score(data, n_samples=S, seed=SEED, max_grid=0)


# ------------------------------------------------------------------ thinning
@pytest.mark.parametrize("rate", [0.5, float(np.float32(0.3))])
def test_split(rate):
    _, data, _ = _corpus(701)
    kept, rest = thin.split(data, rate, SEED)
    assert 0 < int(kept.indices.numel()) and 0 < int(rest.indices.numel())
    for g in GRIDS:
        k2, r2 = thin.split(data, rate, SEED, max_grid=g)
        _same_csr(k2, kept)
        _same_csr(r2, rest)
    with pytest.raises(ValueError):
        thin.split(data, rate, SEED, max_grid=0)


@pytest.mark.parametrize("K", [20, 130])
def test_thin_by_topic(K):
    """The responsibility of the last topic: K = 130 puts it in the theta row's third block of
    64 lanes."""
    X, data, _ = _corpus(701)
    rng = np.random.default_rng(K)
    thetas = torch.from_numpy(rng.dirichlet(np.full(K, 0.3), X.shape[0]).astype(np.float32)).cuda()
    tw = torch.from_numpy(rng.gamma(0.5, 1.0, (K, 701)).astype(np.float32)).cuda()
    kept, p = thin.thin_by_topic(data, thetas, tw, K - 1, SEED, return_p=True)
    assert 0 < int(kept.indices.numel()) < int(data.indices.numel())
    assert float(p.min()) >= 0 and float(p.max()) <= 1 and int((p > 0).sum()) > 0
    for g in GRIDS:
        k2, p2 = thin.thin_by_topic(data, thetas, tw, K - 1, SEED, return_p=True, max_grid=g)
        assert torch.equal(torch.diff(k2.indptr), torch.diff(kept.indptr))      # kept counts per row
        assert torch.equal(p2, p)
        _same_csr(k2, kept)


# ------------------------------------------------------------------ co-occurrence
def test_cooccurrence_pack_groups():
    """300 documents: G = 5 groups of 64 on a pack grid of 1 and 3."""
    X = random_csr(300, 700, 40)
    data = DeviceCSR(X, "cuda")
    words = np.random.default_rng(128).permutation(700)[:128]
    base = cooccurrence_counts(data, words, engine="fused")
    xb = (X[:, words] > 0).astype(np.int64)
    assert torch.equal(base.cpu(), torch.from_numpy(np.asarray((xb.T @ xb).todense())))
    for g in GRIDS:
        assert torch.equal(cooccurrence_counts(data, words, engine="fused", max_grid=g), base), g
    with pytest.raises(ValueError):
        cooccurrence_counts(data, words, engine="fused", max_grid=0)
