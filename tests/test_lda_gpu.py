"""Gibbs LDA on the fused engine (csrc/gibbs.hip): the teacher-forced sweep oracle on every
topic-per-lane width, the count identities, bitwise independence of grid / chunk / recount
split, the initial state against the twin, and quality."""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import DeviceCSR
from gfedntm_amd.ops import lda
from tests import lda_oracle as lo
from tests.test_lda import (BETA, KS, SEED, asym_alpha, check_counts, check_sweeps, corpus, fit_score,
                            zero_draw_sweep)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def data():
    return DeviceCSR(corpus(), "cuda:0")


@pytest.mark.parametrize("K", KS)
def test_sweep_oracle_fused(K):
    assert check_sweeps(corpus(), K, "fused") == [0, 0, 0]


@pytest.mark.parametrize("K,kw", [(3, {}), (130, {}), (65, dict(seg=16, max_grid=2, chunk=37))])
def test_count_identities_fused(data, K, kw):
    check_counts(corpus(), K, "fused", data=data, **kw)


@pytest.mark.parametrize("K", [3, 130, 512])
def test_determinism(data, K):
    alpha = asym_alpha(K)

    def run(seed=SEED, **kw):
        s = lda.GibbsSampler(data, K, alpha, BETA, seed, **kw).sweep(3)
        return s.z.clone(), s.ndk.clone(), s.nwk.clone()

    base = run()
    for kw in (dict(max_grid=1), dict(max_grid=3), dict(chunk=37), dict(seg=16), {}):
        got = run(**kw)
        assert all(torch.equal(a, b) for a, b in zip(base, got)), kw
    assert not torch.equal(base[0], run(seed=SEED + 1)[0])


@pytest.mark.parametrize("K", KS)
def test_initial_state_equals_the_twin(data, K):
    host = lda.GibbsSampler(corpus(), K, 0.1, BETA, SEED, engine="host", doc0=5)
    for kw in ({}, dict(chunk=37, max_grid=2)):
        dev = lda.GibbsSampler(data, K, 0.1, BETA, SEED, doc0=5, **kw)
        assert torch.equal(dev.z.cpu(), host.z)
        assert torch.equal(dev.nwk.cpu(), host.nwk) and torch.equal(dev.ndk.cpu(), host.ndk)


def test_zero_draw_passes_over_zero_probability_topics():
    """u = 0 in front of two topics of probability 0 (tests/test_lda.py ZERO_DRAW): the
    kernel's ``cum <= target`` count lands on the first topic that can be drawn."""
    assert zero_draw_sweep("fused") == (0, 2)


def test_corpus_without_tokens():
    import scipy.sparse as sp
    s = lda.GibbsSampler(sp.csr_matrix((3, 7), dtype=np.float32), 4, 0.1, engine="fused").sweep(2)
    assert s.N == 0 and int(s.nk.sum()) == 0 and int(s.ndk.sum()) == 0


def test_quality_small_fused():
    csr, phi, ref = lo.small_case()
    got = fit_score(csr, phi, lo.SMALL["K"], "fused")
    print("serial", ref, "fused", got)
    assert got >= ref - 0.02


def test_quality_medium_fused():
    csr, phi = lo.lda_corpus(seed=0, **lo.MEDIUM)
    got = fit_score(csr, phi, lo.MEDIUM["K"], "fused")
    print("serial two-seed minimum", lo.MEDIUM_SERIAL_MIN, "fused", got)
    assert got >= lo.MEDIUM_SERIAL_MIN - 0.05


def test_fold_in_and_model_on_the_device():
    from gfedntm_amd.data.bow import BOWDataset
    from gfedntm_amd.models import GibbsLDA
    csr, phi = lo.lda_corpus(seed=1, **lo.SMALL)
    ds = BOWDataset(csr, {i: "w%d" % i for i in range(csr.shape[1])})
    m = GibbsLDA(3, alpha=0.3, beta=0.02, num_iterations=60, optimize_interval=10, burn_in=20,
                 seed=2, device="cuda:0").fit(ds)
    assert m.engine_info()["engine"] == "fused"
    tw, th = m.get_topic_word_distribution(), m.get_doc_topic_distribution(ds)
    assert np.allclose(tw.sum(1), 1, atol=1e-9) and np.allclose(th.sum(1), 1, atol=1e-9)
    nwk = m.sampler.nwk.clone()
    fold = m.get_doc_topic_distribution(BOWDataset(csr, ds.idx2token), n_samples=40)
    assert torch.equal(m.sampler.nwk, nwk)
    assert np.abs(fold - th).mean() < 0.1 and (fold.argmax(1) == th.argmax(1)).mean() > 0.8
