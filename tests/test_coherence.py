"""Topic coherence from exact integer co-occurrence counts, on the CPU: the counts against
the scipy product, NPMI from counts against ``npmi_coherence`` (bit for bit), the model
and federation APIs, two gloo ranks, the CLI."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BOWDataset, DeviceCSR
from gfedntm_amd.data.synthetic import generate_synthetic
from gfedntm_amd.eval.metrics import (cooccurrence_counts, federated_cooccurrence, npmi_coherence,
                                      npmi_from_counts, topic_diversity)
from gfedntm_amd.federation.data import ClientCorpus
from gfedntm_amd.federation.runner import LocalFederation
from gfedntm_amd.models import AVITM
from gfedntm_amd.utils.config import load_config
from tests.helpers import random_csr

VOCAB = {i: str(i) for i in range(1024)}


def oracle_counts(X, words):
    xb = (X[:, list(words)] > 0).astype(np.int64)
    return np.asarray((xb.T @ xb).todense())


@pytest.fixture(scope="module")
def corpus():
    return random_csr(300, 700, 40)


@pytest.fixture(scope="module")
def topics():
    """20 topics x 10 words over V = 700, overlapping (fewer than 200 distinct words)."""
    rng = np.random.default_rng(3)
    pool = rng.choice(700, size=180, replace=False)
    return [list(map(int, rng.choice(pool, size=10, replace=False))) for _ in range(20)]


@pytest.mark.parametrize("as_device_csr", [False, True])
def test_exact_counts_match_scipy_product(corpus, topics, as_device_csr):
    words = sorted({w for t in topics for w in t})
    shuffled = list(np.random.default_rng(0).permutation(words))
    data = DeviceCSR(corpus, "cpu") if as_device_csr else corpus
    for ws in (words, shuffled):
        got = cooccurrence_counts(data, ws, engine="exact")
        assert got.dtype == torch.int64 and got.shape == (len(ws), len(ws))
        assert got.device.type == "cpu"
        assert np.array_equal(got.numpy(), oracle_counts(corpus, ws))
    # the default engine off the GPU is the exact one; a tensor of words is taken as well
    assert torch.equal(cooccurrence_counts(data, torch.tensor(shuffled)), got)


def test_stored_zeros_do_not_count():
    X = sp.csr_matrix((np.array([1, 0, 2, 3, 0], dtype=np.float32), np.array([0, 1, 2, 0, 2]),
                       np.array([0, 3, 5])), shape=(2, 3))
    got = cooccurrence_counts(X, [0, 1, 2], engine="exact").numpy()
    assert np.array_equal(got, [[2, 0, 1], [0, 0, 0], [1, 0, 1]])


def test_bad_words_raise(corpus):
    for bad in ([1, 2, 2], [0, 700], [-1, 3]):
        with pytest.raises(ValueError):
            cooccurrence_counts(corpus, bad, engine="exact")
    with pytest.raises(ValueError):
        cooccurrence_counts(corpus, [1, 2], engine="dense")
    with pytest.raises(RuntimeError):                  # the kernels need the data on a GPU
        cooccurrence_counts(DeviceCSR(corpus, "cpu"), [1, 2], engine="fused")


def test_npmi_from_counts_is_bitwise_npmi_coherence(corpus, topics):
    words = list(np.random.default_rng(1).permutation(sorted({w for t in topics for w in t})))
    counts = cooccurrence_counts(corpus, words, engine="exact")
    got = npmi_from_counts(topics, words, counts, corpus.shape[0], per_topic=True)
    ref = npmi_coherence(topics, corpus, per_topic=True)
    assert got == ref
    assert npmi_from_counts(topics, words, counts, corpus.shape[0]) == npmi_coherence(topics, corpus)


def test_npmi_from_counts_degenerate_pairs():
    # words 0, 1 always co-occur; word 2 never with them; word 3 never occurs
    X = sp.csr_matrix(np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]],
                               dtype=np.float32))
    words = [3, 0, 2, 1]
    counts = cooccurrence_counts(X, words, engine="exact")
    for t in ([[0, 1]], [[0, 2]], [[0, 3]], [[0, 1, 2, 3], [2, 3]]):
        got = npmi_from_counts(t, words, counts, 4, per_topic=True)
        ref = npmi_coherence(t, X, per_topic=True)
        assert got == ref or (np.isnan(got).all() and np.isnan(ref).all())
    assert abs(npmi_from_counts([[0, 1]], words, counts, 4) - 1.0) < 1e-6
    assert npmi_from_counts([[0, 2]], words, counts, 4) < -0.9


def _avitm(model_type, X, seed=0):
    torch.manual_seed(seed)
    tm = AVITM(input_size=X.shape[1], n_components=8, model_type=model_type, hidden_sizes=(16, 12),
               batch_size=32, lr=5e-3, verbose=False, device="cpu", backend="torch")
    ds = BOWDataset(X, VOCAB)
    for ep in range(2):
        tm._train_epoch(ds, seed=ep)
    return tm, ds


def test_model_coherence_matches_oracle(corpus):
    tm, ds = _avitm("prodLDA", corpus)
    got = tm.coherence(ds)
    top = torch.topk(tm.model.beta.detach(), 10, dim=1).indices.numpy()
    assert np.array_equal(got["topics"], top)
    assert got["per_topic"] == npmi_coherence(top, ds.csr, per_topic=True)
    assert got["npmi"] == npmi_coherence(top, ds.csr)
    assert got["diversity"] == topic_diversity(top.tolist(), 10)
    assert got["n_docs"] == 300 and got["engine"] == "exact"
    assert tm.coherence(ds, per_topic=True)["npmi"] == got["per_topic"]
    # ProdLDA's decoder multiplies by beta itself
    dec = tm.coherence(ds, matrix="decoder")
    assert np.array_equal(dec["topics"], top) and dec["per_topic"] == got["per_topic"]
    # another top-k, and the training data by default
    tm.train_data = ds
    top5 = top[:, :5]
    assert tm.coherence(topk=5)["per_topic"] == npmi_coherence(top5, ds.csr, per_topic=True)
    with pytest.raises(ValueError):
        tm.coherence(ds, matrix="theta")


def test_neural_lda_decoder_matrix(corpus):
    tm, ds = _avitm("LDA", corpus)
    beta = tm.model.beta.detach().double()
    bn = (beta - beta.mean(0, keepdim=True)) / torch.sqrt(
        beta.var(0, unbiased=False, keepdim=True) + tm.model.beta_batchnorm.eps)
    direct = torch.topk(torch.softmax(bn, dim=1), 10, dim=1).indices.numpy()
    top = torch.topk(tm.topic_word_matrix_tensor(), 10, dim=1).indices.numpy()
    assert np.array_equal(np.sort(top, 1), np.sort(direct, 1))
    got = tm.coherence(ds, matrix="decoder")
    assert np.array_equal(got["topics"], top)
    assert got["per_topic"] == npmi_coherence(top, ds.csr, per_topic=True)
    raw = torch.topk(tm.model.beta.detach(), 10, dim=1).indices.numpy()
    assert not np.array_equal(raw, top)                 # column batch-norm reorders the words
    assert np.array_equal(tm.coherence(ds)["topics"], raw)


# ---------------------------------------------------------------------------------- federation
def _params(**kw):
    p = dict(load_config().training_params)
    p.update(num_epochs=2, batch_size=16, hidden_sizes=(16, 16), n_components=5)
    p.update(kw)
    return p


def _corpora(n=3, seed=1):
    sc = generate_synthetic(vocab_size=120, n_topics=5, n_docs=40, n_nodes=n, frozen_topics=2,
                            nwords=(15, 30), seed=seed)
    return [ClientCorpus(synthetic=sc, node=i) for i in range(n)]


def _vstack_oracle(fed, topk=10):
    tm = fed.clients[0].tm
    top = torch.topk(tm.model.beta.detach(), topk, dim=1).indices.cpu().numpy()
    X = sp.vstack([c.dataset.csr for c in fed.clients], format="csr")
    return top, X, npmi_coherence(top, X, per_topic=True)


def test_local_federation_coherence():
    corpora = _corpora(3)
    assert len({tuple(c.local_terms()) for c in corpora}) == 3       # different local vocabularies
    fed = LocalFederation(corpora, _params(), max_iters=4, device="cpu", backend="torch", seed=2)
    fed.run()
    got = fed.coherence()
    top, X, ref = _vstack_oracle(fed)
    assert got["per_topic"] == ref and got["npmi"] == float(np.mean(ref))
    assert got["n_docs"] == X.shape[0] == sum(c.n_docs for c in fed.clients)
    assert got["clients"] == 3 and got["engine"] == "exact"
    assert np.array_equal(got["topics"], top)
    assert got["diversity"] == topic_diversity(top.tolist(), 10)


def _count_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X = random_csr(300, 700, 40)
        words = list(np.random.default_rng(5).choice(700, size=150, replace=False))
        half = X[:130] if rank == 0 else X[130:]
        counts, n_docs = federated_cooccurrence([half], words)
        local, n_local = federated_cooccurrence([half], words, group=False)
        corpus = _corpora(world)[rank]
        from gfedntm_amd.federation.runner import run_distributed
        out = run_distributed(corpus, _params(), max_iters=4, backend="torch", seed=2,
                              coherence_topk=10)
        plain = run_distributed(corpus, _params(), max_iters=4, backend="torch", seed=2)
        q.put((rank, counts.numpy(), n_docs, local.numpy(), n_local, out["npmi"], out["npmi_topk"],
               out["topic_diversity"], sorted(k for k in plain if "npmi" in k or "diversity" in k)))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_count_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X = random_csr(300, 700, 40)
    words = list(np.random.default_rng(5).choice(700, size=150, replace=False))
    whole = oracle_counts(X, words)
    for rank, counts, n_docs, local, n_local, *_ in res:
        assert np.array_equal(counts, whole) and n_docs == 300
        part = X[:130] if rank == 0 else X[130:]
        assert np.array_equal(local, oracle_counts(part, words)) and n_local == part.shape[0]
    # the same federation in one process
    fed = LocalFederation(_corpora(2), _params(), max_iters=4, device="cpu", backend="torch", seed=2)
    fed.run()
    coh = fed.coherence()
    for r in res:
        assert r[5] == res[0][5] == coh["npmi"] and np.isfinite(r[5])
        assert r[6] == 10 and r[7] == coh["diversity"]
        assert r[8] == []                               # coherence_topk=0: no extra keys


# ---------------------------------------------------------------------------------- CLI
def test_cli_npmi(tmp_path):
    from gfedntm_amd.cli import main
    base = ["--workdir", str(tmp_path), "--min_clients_federation", "2", "--max_iters", "4",
            "--engine", "torch", "--device", "cpu", "--generate_synthetic", str(tmp_path / "syn.npz")]
    with pytest.raises(SystemExit):
        main(base + ["--npmi_topk", "10", "--backend", "grpc"])
    out = main(base + ["--npmi_topk", "10"])
    assert out["rounds"] == 4 and out["npmi_topk"] == 10
    assert np.isfinite(out["npmi"]) and 0 < out["topic_diversity"] <= 1
    assert "npmi" not in main(base)
