"""Gibbs LDA on the host engine (the numpy twin of csrc/gibbs.hip): the teacher-forced sweep
oracle and the mutants that pin it, the count identities, quality against the textbook
serial sampler, GibbsLDA and the wrapper's "gibbs" trainer."""
import json

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

from gfedntm_amd.data.bow import BOWDataset
from gfedntm_amd.experiments.tm_wrapper import TMWrapper
from gfedntm_amd.models import GibbsLDA
from gfedntm_amd.ops import lda, srchash
from tests import lda_oracle as lo
from tests.helpers import row_edge_csr

KS = [3, 64, 65, 130, 512]
BETA, SEED = 0.01, 11


def corpus():
    csr, _ = row_edge_csr(701)
    return csr


def asym_alpha(K):
    """An asymmetric prior: 0.05 .. 0.6, no two neighbours equal."""
    return (0.05 + 0.55 * ((np.arange(K) * 7) % K) / K).astype(np.float32)


def state(s):
    """Copies of a chain's (z, nwk, nk) as numpy."""
    return (s.z.cpu().numpy()[:s.N].astype(np.int64), s.nwk.cpu().numpy().copy(),
            s.nk.cpu().numpy().copy())


def check_sweeps(csr, K, engine, **kw):
    """The sweep oracle from the initial state and from the state three sweeps later, then a
    frozen chain against the trained counts.  Returns the rejected tokens of each."""
    tok = lo.Tokens(csr)
    alpha = asym_alpha(K)
    s = lda.GibbsSampler(csr, K, alpha, BETA, SEED, engine=engine, **kw)
    out = []
    for lead in (0, 2):
        s.sweep(lead)
        z0, nwk0, nk0 = state(s)
        s.sweep()
        out.append(lo.sweep_rejects(tok, z0, state(s)[0], nwk0, nk0, alpha, BETA, SEED, s.sweeps))
    nwk, nk = s.nwk.clone(), s.nk.clone()
    f = lda.GibbsSampler(csr, K, alpha, BETA, SEED + 1, engine=engine, counts=(s.nwk, s.nk), **kw)
    z0 = state(f)[0]
    f.sweep()
    out.append(lo.sweep_rejects(tok, z0, state(f)[0], nwk.cpu().numpy(), nk.cpu().numpy(), alpha,
                                BETA, SEED + 1, 1, frozen=True))
    assert torch.equal(f.nwk, nwk) and torch.equal(f.nk, nk)          # frozen: never rewritten
    assert torch.equal(s.nwk, nwk) and torch.equal(s.nk, nk)
    return out


def check_counts(csr, K, engine, data=None, **kw):
    """nwk, nk, ndk against bincounts of z after the initialisation and after each of three
    sweeps, exactly (``data``: the same corpus as the sampler shall take it)."""
    tok = lo.Tokens(csr)
    s = lda.GibbsSampler(csr if data is None else data, K, asym_alpha(K), BETA, SEED, engine=engine, **kw)
    for _ in range(4):
        z = s.z.cpu().numpy()[:s.N]
        assert z.min() >= 0 and z.max() < K
        nwk, nk, ndk = (torch.from_numpy(a.astype(np.int32)) for a in lo.counts(tok, z, K))
        assert torch.equal(s.nwk.cpu(), nwk)
        assert torch.equal(s.nk.cpu(), nk) and torch.equal(s.nk.cpu(), s.nwk.cpu().sum(0, dtype=torch.int32))
        assert torch.equal(s.ndk.cpu(), ndk)
        assert int(s.nk.sum()) == tok.N == s.N
        s.sweep()


def test_philox_and_initial_state():
    csr = corpus()
    tok = lo.Tokens(csr)
    u = lda.host_draws(SEED, 3, 5 + tok.doc, tok.pos)
    assert np.array_equal(u.astype(np.float64), lo.draws(SEED, 3, 5 + tok.doc, tok.pos))
    for K in KS:
        s = lda.GibbsSampler(csr, K, 0.1, BETA, SEED, engine="host", doc0=5)
        assert np.array_equal(state(s)[0], lo.initial_z(tok, K, SEED, doc0=5))


@pytest.mark.parametrize("K", KS)
def test_sweep_oracle_host(K):
    assert check_sweeps(corpus(), K, "host") == [0, 0, 0]


@pytest.mark.parametrize("variant", ["no_exclusion", "alpha_shift", "no_decrement", "live_nk"])
def test_oracle_rejects_mutant(variant):
    """The oracle must reject each wrong sampler.  Measured on this corpus (K = 65, three
    sweeps, 33 687 tokens): no_exclusion 6694, alpha_shift 3008, no_decrement 2184, live_nk
    3116 tokens rejected."""
    csr, K = corpus(), 65
    tok = lo.Tokens(csr)
    alpha = asym_alpha(K)
    s = lda.GibbsSampler(csr, K, alpha, BETA, SEED, engine="host")
    bad = 0
    for _ in range(3):
        z0, nwk0, nk0 = state(s)
        s.sweep(_variant=(variant,))
        bad += lo.sweep_rejects(tok, z0, state(s)[0], nwk0, nk0, alpha, BETA, SEED, s.sweeps)
    print(variant, "rejected tokens:", bad)
    assert bad > 0


# ``<`` for ``<=`` in the search differs from the sampler only where cum_k == target exactly, and
# the oracle can tell the two apart only where that tie is at 0: a draw that is exactly 0 in
# front of topics of probability exactly 0.  On the corpus above neither occurs (the mutant's z
# is the twin's bit for bit), so this case builds one: with seed 11, token 0 of global document
# 25 859 526 draws the Philox word 155 in sweep 1, u = 0; that document has one token, and
# alpha_0 = alpha_1 = 0, so once its token is taken out p_0 = p_1 = 0 and cum_0 = cum_1 = 0 =
# target.  ``<=`` passes over both and lands on topic 2; ``<`` picks topic 0, which has
# probability 0.
ZERO_DRAW = dict(seed=11, doc0=25859526, K=4, alpha=np.array([0.0, 0.0, 0.3, 0.2], np.float32))


def zero_draw_corpus():
    x = np.zeros((40, 9), dtype=np.float32)
    x[0, 4] = 1
    rng = np.random.default_rng(3)
    for d in range(1, 40):
        x[d] = rng.multinomial(12, np.full(9, 1 / 9))
    return sp.csr_matrix(x)


def zero_draw_sweep(engine, variant=()):
    """(rejected tokens, the new topic of the token whose draw is 0) of sweep 1."""
    c = ZERO_DRAW
    csr = zero_draw_corpus()
    tok = lo.Tokens(csr)
    assert lo.draws(c["seed"], 1, [c["doc0"]], [0])[0] == 0.0
    s = lda.GibbsSampler(csr, c["K"], c["alpha"], BETA, c["seed"], engine=engine, doc0=c["doc0"])
    z0, nwk0, nk0 = state(s)
    s.sweep(_variant=variant)
    z1 = state(s)[0]
    bad = lo.sweep_rejects(tok, z0, z1, nwk0, nk0, c["alpha"], BETA, c["seed"], 1, doc0=c["doc0"])
    return bad, int(z1[0])


def test_oracle_rejects_mutant_strict():
    assert zero_draw_sweep("host") == (0, 2)
    bad, k = zero_draw_sweep("host", ("strict",))
    print("strict rejected tokens:", bad, "topic", k)
    assert k == 0 and bad > 0


@pytest.mark.parametrize("K", [3, 130])
def test_count_identities_host(K):
    check_counts(corpus(), K, "host")


def test_engine_and_argument_checks():
    csr = corpus()
    with pytest.raises(ValueError):
        lda.GibbsSampler(csr, 513, 0.1, engine="host")
    with pytest.raises(ValueError):
        lda.GibbsSampler(csr, 4, np.array([0.1, 0.1, -0.1, 0.1]), engine="host")
    with pytest.raises(ValueError):
        lda.GibbsSampler(csr, 4, np.zeros(4), engine="host")
    with pytest.raises(ValueError):
        lda.GibbsSampler(csr * 0.5, 4, 0.1, engine="host")
    with pytest.raises(ValueError):
        lda.GibbsSampler(csr, 4, 0.1, engine="gpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            lda.GibbsSampler(csr, 4, 0.1, engine="fused")
    a = lda.GibbsSampler(csr, 5, 0.1, seed=3, engine="host").sweep(2)
    b = lda.GibbsSampler(csr, 5, 0.1, seed=3, engine="host").sweep(2)
    c = lda.GibbsSampler(csr, 5, 0.1, seed=4, engine="host").sweep(2)
    assert torch.equal(a.z, b.z) and not torch.equal(a.z, c.z)
    empty = lda.GibbsSampler(sp.csr_matrix((3, 7), dtype=np.float32), 4, 0.1, engine="host").sweep()
    assert empty.N == 0 and int(empty.nk.sum()) == 0


def test_source_hash_follows_the_kernel(tmp_path):
    assert "gibbs.hip" in srchash.KERNEL_SRCS
    import os
    import shutil
    dst = tmp_path / "csrc"
    shutil.copytree(srchash.CSRC, dst)
    assert srchash.source_hash(csrc=str(dst)) == srchash.source_hash()
    with open(os.path.join(dst, "gibbs.hip"), "a") as f:
        f.write("// touched\n")
    assert srchash.source_hash(csrc=str(dst)) != srchash.source_hash()


def fit_score(csr, phi, K, engine, seed=0):
    m = GibbsLDA(K, alpha=lo.QUALITY["alpha"] * K, beta=lo.QUALITY["beta"],
                 num_iterations=lo.QUALITY["sweeps"], optimize_interval=0, seed=seed, engine=engine)
    m.fit(BOWDataset(csr, {i: str(i) for i in range(csr.shape[1])}))
    return lo.score(phi, m.get_topic_word_distribution())


def test_quality_small_host():
    csr, phi, ref = lo.small_case()
    got = fit_score(csr, phi, lo.SMALL["K"], "host")
    print("serial", ref, "host", got)
    assert got >= ref - 0.02


def test_gibbs_lda_model():
    csr, phi = lo.lda_corpus(seed=1, **lo.SMALL)
    ds = BOWDataset(csr, {i: "w%d" % i for i in range(csr.shape[1])})
    m = GibbsLDA(3, alpha=0.3, beta=0.02, num_iterations=60, optimize_interval=0, seed=2,
                 engine="host").fit(ds)
    assert m.engine_info()["engine"] == "host"
    tw, th = m.get_topic_word_distribution(), m.get_doc_topic_distribution(ds)
    assert tw.shape == (3, 20) and th.shape == (60, 3)
    assert np.allclose(tw.sum(1), 1, atol=1e-9) and np.allclose(th.sum(1), 1, atol=1e-9)
    s = m.sampler
    assert np.allclose(tw, ((s.nwk.numpy() + s.beta) / (s.nk.numpy() + 20 * s.beta)).T)
    assert np.allclose(th, (s.ndk.numpy() + m.alphas) / (s.ndk.numpy().sum(1, keepdims=True) + m.alphas.sum()))
    topics = m.get_topics(5)
    assert len(topics) == 3 and all(len(t) == 5 and t[0].startswith("w") for t in topics)
    # fold-in of the training documents (as an unseen corpus) lands near their training theta
    fold = m.get_doc_topic_distribution(BOWDataset(csr, ds.idx2token), n_samples=40)
    assert np.allclose(fold.sum(1), 1, atol=1e-9)
    assert np.abs(fold - th).mean() < 0.1 and (fold.argmax(1) == th.argmax(1)).mean() > 0.8


def test_alpha_optimisation_finds_the_dominant_topic():
    # three topics on disjoint word sets, documents drawn with the prior (2.0, 0.2, 0.2): the
    # first topic dominates, and the fixed point must find the asymmetry
    rng = np.random.default_rng(0)
    phi = np.zeros((3, 30))
    for k in range(3):
        phi[k, 10 * k:10 * k + 10] = 0.1
    x = np.zeros((120, 30), dtype=np.float32)
    for d in range(120):
        x[d] = rng.multinomial(40, rng.dirichlet([2.0, 0.2, 0.2]) @ phi)
    m = GibbsLDA(3, alpha=1.5, beta=0.02, num_iterations=60, optimize_interval=1, burn_in=20,
                 seed=0, engine="host").fit(BOWDataset(sp.csr_matrix(x), {i: str(i) for i in range(30)}))
    tw = m.get_topic_word_distribution()
    dominant = int(tw[:, :10].sum(1).argmax())
    assert tw[dominant, :10].sum() > 0.9
    assert int(m.alphas.argmax()) == dominant
    assert m.alphas[dominant] > 2 * np.delete(m.alphas, dominant).max()
    assert np.array_equal(m.sampler.alpha, m.alphas)


WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda omicron sigma "
         "tau upsilon omega river mountain forest ocean").split()


def test_wrapper_gibbs_trainer(tmp_path):
    rng = np.random.default_rng(0)
    docs = [" ".join(rng.choice(WORDS, size=rng.integers(10, 25))) for _ in range(60)]
    pq = tmp_path / "corpus.parquet"
    pd.DataFrame({"id": range(60), "bow_text": docs}).to_parquet(pq)
    params = dict(ntopics=3, alpha=5.0, optimize_interval=10, num_iterations=30, thetas_thr=3e-3,
                  doc_topic_thr=0.0, num_threads=4, hidden_sizes=(16, 16))
    w = TMWrapper(device="cpu")
    root = w.train_root_model(str(tmp_path / "models"), "root", str(pq), "gibbs", params)
    tmd = root / "TMmodel"
    betas, thetas = np.load(tmd / "betas.npy"), sp.load_npz(tmd / "thetas.npz")
    vocab = (tmd / "vocab.txt").read_text().split()
    assert betas.shape == (3, len(vocab)) and np.allclose(betas.sum(1), 1, atol=1e-6)
    assert thetas.shape == (60, 3) and np.allclose(thetas.sum(1), 1, atol=1e-5)
    alphas = np.load(tmd / "alphas.npy")
    assert alphas.shape == (3,) and np.all(alphas > 0)
    assert len((tmd / "tpc_descriptions.txt").read_text().strip().split("\n")) == 3
    assert np.load(tmd / "topic_coherence.npy").shape == (3,)
    cfg = json.loads((root / "config.json").read_text())
    assert cfg["trainer"] == "gibbs" and cfg["TMparam"]["num_iterations"] == 30
    assert "hidden_sizes" not in cfg["TMparam"] and cfg["TMparam"]["alpha"] == 5.0
    th = thetas.toarray()
    params2 = dict(params, ntopics=2, optimize_interval=0)
    sub = w.train_htm_submodel("HTM-DS", root, "sub_ds", "gibbs", params2, expansion_topic=1, thr=0.2)
    assert len(pd.read_parquet(sub / "corpus.parquet")) == int((th[:, 1] > 0.2).sum()) > 0
    assert np.load(sub / "TMmodel" / "betas.npy").shape[0] == 2
    assert np.allclose(np.load(sub / "TMmodel" / "alphas.npy"), 2.5)          # 5 / K, not optimised
    with pytest.raises(NotImplementedError, match="gibbs"):
        w.train_root_model(str(tmp_path / "models"), "m", str(pq), "mallet", params)
