"""Word co-occurrence kernels (csrc/cooc.hip) against the exact integer oracle (the scipy
product of the binarised columns).  Counts are integers: every comparison is
``torch.equal``, there are no tolerances."""
import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BatchPlan, BOWDataset, DeviceCSR
from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.eval.metrics import cooccurrence_counts, npmi_coherence
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.federation.runner import LocalFederation
from gfedntm_amd.models import AVITM
from gfedntm_amd.ops import cooc, kernel_abi as abi, native
from gfedntm_amd.utils.config import load_config
from tests.helpers import random_csr

pytestmark = pytest.mark.gpu

VOCAB = {i: str(i) for i in range(1024)}


def oracle_counts(X, words):
    xb = (sp.csr_matrix(X)[:, np.asarray(words)] > 0).astype(np.int64)
    return xb.T @ xb                                   # sparse int64 [W, W]


def assert_counts(got, X, words):
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == (len(words), len(words))
    ref = torch.from_numpy(np.asarray(oracle_counts(X, words).todense()))
    assert torch.equal(got.cpu(), ref)


@pytest.fixture(scope="module")
def corpus():
    return random_csr(300, 700, 40)


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


# tail groups of documents (D % 64), tail tiles of words (W % 64), one tile on the diagonal
@pytest.mark.parametrize("D", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 200])
def test_counts_match_oracle(corpus, D, W):
    X = corpus[:D]
    words = np.random.default_rng(W).permutation(700)[:W]      # distinct, in shuffled order
    assert_counts(cooccurrence_counts(DeviceCSR(X, "cuda"), words, engine="fused"), X, words)


def test_edge_rows():
    """70 documents: an empty first and last one, one with none of the words, one with all of
    them, one with 400 non-zeros; then stored values set to 0 on the device stop counting."""
    rng = np.random.default_rng(2)
    V, W = 700, 90
    words = rng.permutation(V)[:W]
    others = np.setdiff1d(np.arange(V), words)
    X = random_csr(70, V, 40, seed=5).tolil()
    X[0, :] = 0
    X[69, :] = 0
    X[7, :] = 0
    X[7, others[:30]] = 1.0                               # none of the words
    X[8, :] = 0
    X[8, words] = 2.0                                     # all of them
    X[9, :] = 0
    X[9, rng.permutation(V)[:400]] = 3.0                  # a long row
    X = sp.csr_matrix(X, dtype=np.float32)
    X.eliminate_zeros()
    X.sort_indices()
    assert X[0].nnz == X[69].nnz == 0 and X[9].nnz == 400
    data = DeviceCSR(X, "cuda")
    assert_counts(cooccurrence_counts(data, words, engine="fused"), X, words)
    # stored zeros: every third entry zeroed in place on the device
    data.values[::3] = 0.0
    Z = X.copy()
    Z.data[::3] = 0.0
    assert Z.nnz == X.nnz                                 # the entries stay stored
    got = cooccurrence_counts(data, words, engine="fused")
    assert_counts(got, Z, words)
    assert not torch.equal(got.cpu(), torch.from_numpy(np.asarray(oracle_counts(X, words).todense())))


def test_chunk_independence(corpus):
    words = np.random.default_rng(9).permutation(700)[:200]
    data = DeviceCSR(corpus, "cuda")
    base = cooccurrence_counts(data, words, engine="fused")
    assert_counts(base, corpus, words)
    for chunk in (100, 64, 1):
        assert torch.equal(cooccurrence_counts(data, words, engine="fused", chunk=chunk), base)
    assert torch.equal(cooccurrence_counts(data, words), base)          # the default engine
    with pytest.raises(ValueError):
        cooccurrence_counts(data, words, engine="fused", chunk=0)
    with pytest.raises(ValueError):
        cooccurrence_counts(data, [3, 3], engine="fused")


def _big_csr(D, V, nnz, seed):
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, V, size=(D, nnz))
    rows = np.repeat(np.arange(D), nnz)
    X = sp.csr_matrix((np.ones(D * nnz, dtype=np.float32), (rows, cols.ravel())), shape=(D, V))
    X.sum_duplicates()
    X.sort_indices()
    return X


def test_many_documents_no_dense_matrix():
    """More than 65 535 documents; the peak device memory of the call stays below the bytes
    of the dense [D, W] fp32 operand alone."""
    D, V, W = 70_000, 4466, 128
    X = _big_csr(D, V, 20, seed=3)
    words = np.random.default_rng(4).permutation(V)[:W]
    data = DeviceCSR(X, "cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = cooccurrence_counts(data, words, engine="fused")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print("peak bytes", peak, "dense operand", 4 * D * W)
    assert peak < 4 * D * W
    assert_counts(got, X, words)
    assert torch.equal(cooccurrence_counts(data, words, engine="fused", chunk=30_001), got)


def _assert_sparse_equal(got, ref):
    """got (dense, device) == ref (scipy sparse) without a second dense matrix."""
    ref = ref.tocoo()
    ref.eliminate_zeros()
    g = got.cpu().numpy()
    assert np.count_nonzero(g) == ref.nnz
    assert np.array_equal(g[ref.row, ref.col], ref.data)


def test_word_limit():
    limit = cooc.max_words()
    assert limit >= 5120                                  # K = 512 topics x 10 words
    V = limit + 56
    X = random_csr(100, V, 60, seed=8)
    data = DeviceCSR(X, "cuda")
    perm = np.random.default_rng(1).permutation(V)
    at = perm[:limit]
    _assert_sparse_equal(cooccurrence_counts(data, at, engine="fused"), oracle_counts(X, at))
    over = perm[:limit + 1]
    with pytest.raises(ValueError):
        cooccurrence_counts(data, over, engine="fused")
    from gfedntm_amd.eval.metrics import _cooccurrence
    got, engine = _cooccurrence(data, over, None, None)   # past the limit: the host product
    assert engine == "exact" and got.is_cuda
    _assert_sparse_equal(got, oracle_counts(X, over))
    del got
    assert _cooccurrence(data, at[:64], None, None)[1] == "fused"


def test_launcher_checks(corpus):
    """Bad parameter structs return the launcher's negative codes; nothing is launched."""
    lib = native.kernels()
    assert lib.gfk_cooc_struct_size() == C.sizeof(abi.GfkCooc)
    data = DeviceCSR(corpus, "cuda")
    W = 8
    slot = torch.full((700,), -1, dtype=torch.int32, device="cuda")
    bits = torch.zeros(W * 5, dtype=torch.int64, device="cuda")
    out = torch.zeros(W, W, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def struct(**kw):
        p = abi.GfkCooc()
        p.indptr, p.indices, p.values = data.indptr.data_ptr(), data.indices.data_ptr(), data.values.data_ptr()
        p.slot, p.bits, p.counts = slot.data_ptr(), bits.data_ptr(), out.data_ptr()
        p.n_docs, p.bits_words, p.W, p.V = 300, W * 5, W, 700
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert lib.gfk_cooc(C.byref(struct(W=0)), stream) == -5
    assert lib.gfk_cooc(C.byref(struct(W=cooc.max_words() + 1)), stream) == -5
    assert lib.gfk_cooc(C.byref(struct(n_docs=1 << 31)), stream) == -6
    assert lib.gfk_cooc(C.byref(struct(n_docs=-1)), stream) == -6
    for field in ("indptr", "indices", "values", "slot", "bits", "counts"):
        assert lib.gfk_cooc(C.byref(struct(**{field: None})), stream) == -7
    assert lib.gfk_cooc(C.byref(struct(bits_words=W * 5 - 1)), stream) == -9
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0 and int(bits.abs().sum()) == 0


def test_model_coherence_fused():
    torch.manual_seed(0)
    X = random_csr(300, 700, 40, seed=1)
    tm = AVITM(input_size=700, n_components=20, hidden_sizes=(32, 24), batch_size=64, verbose=False,
               device="cuda", backend="fused")
    ds = BOWDataset(X, VOCAB)
    tm.engine.bind_data(tm.device_data(ds), BatchPlan.build(300, 64, 5, seed=0))
    for s in range(5):
        tm.engine.step(s)
    torch.cuda.synchronize()
    got = tm.coherence(ds, per_topic=True)
    top = torch.topk(tm.model.beta.detach(), 10, dim=1).indices.cpu().numpy()
    assert got["engine"] == "fused" and got["n_docs"] == 300
    assert np.array_equal(got["topics"], top)
    np.testing.assert_allclose(got["per_topic"], npmi_coherence(top, X, per_topic=True), rtol=1e-12)


def test_local_federation_coherence_fused():
    p = dict(load_config().training_params)
    p.update(num_epochs=2, batch_size=16, hidden_sizes=(16, 16), n_components=10)
    sc = generate_synthetic(vocab_size=400, n_topics=10, n_docs=60, n_nodes=3, frozen_topics=2,
                            nwords=(30, 60), seed=4)
    corpora = [ClientCorpus(synthetic=sc, node=i) for i in range(3)]
    fed = LocalFederation(corpora, p, max_iters=3, device="cuda", backend="fused", seed=1)
    fed.run()
    got = fed.coherence()
    top = torch.topk(fed.clients[0].tm.model.beta.detach(), 10, dim=1).indices.cpu().numpy()
    Xall = sp.vstack([c.dataset.csr for c in fed.clients], format="csr")
    assert got["engine"] == "fused" and got["clients"] == 3 and got["n_docs"] == Xall.shape[0] == 180
    np.testing.assert_allclose(got["per_topic"], npmi_coherence(top, Xall, per_topic=True), rtol=1e-12)
