"""TSS / DSS entry points off the GPU: the engine switch of eval/metrics.py dss / tss /
bhattacharyya, its validation, and TopicModelBase.dss / tss on a CPU torch model against the
host formula on float64 casts.  The kernels themselves: tests/test_simscore_gpu.py."""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BOWDataset
from gfedntm_amd.eval import metrics
from gfedntm_amd.eval.export import postprocess_thetas
from gfedntm_amd.models import AVITM
from tests.helpers import random_csr


def _tss_formula(betas, topic_vectors):
    return float(np.sum(np.max(np.sqrt(betas).dot(np.sqrt(topic_vectors.T)), axis=0)))


def _dss_formula(thetas_true, thetas, n_docs=None):
    n_docs = len(thetas_true) if n_docs is None else n_docs
    a = np.sqrt(thetas_true).dot(np.sqrt(thetas_true.T))
    b = np.sqrt(thetas).dot(np.sqrt(thetas.T))
    return float(np.sum(np.abs(a - b)) / n_docs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("engine", [None, "host"])
def test_host_engines_are_the_formulas(engine, dtype):
    rng = np.random.default_rng(0)
    tt = rng.dirichlet([0.1] * 7, 130).astype(dtype)
    th = rng.dirichlet([0.1] * 5, 130).astype(dtype)
    assert metrics.dss(tt, th, engine=engine) == _dss_formula(tt, th)
    assert metrics.dss(tt, th, 77, engine=engine) == _dss_formula(tt, th, 77)
    b = rng.dirichlet([0.05] * 60, 6).astype(dtype)
    g = rng.dirichlet([0.05] * 60, 4).astype(dtype)
    assert metrics.tss(b, g, engine=engine) == _tss_formula(b, g)
    # CPU tensors are numpy inputs to the host path
    assert metrics.dss(torch.from_numpy(tt), torch.from_numpy(th), engine=engine) == \
        _dss_formula(tt, th)


def test_device_engine_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.full((3, 4), 0.25)
    for call in (lambda: metrics.dss(x, x, engine="device"),
                 lambda: metrics.tss(x, x, engine="device"),
                 lambda: metrics.bhattacharyya(x, x, engine="device")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_engine_names_and_shapes_are_checked():
    x = np.full((3, 4), 0.25)
    for fn in (metrics.dss, metrics.tss, metrics.bhattacharyya):
        with pytest.raises(ValueError, match="engine"):
            fn(x, x, engine="fused")
    with pytest.raises(ValueError, match="documents"):
        metrics.dss(x, np.full((2, 4), 0.25))
    with pytest.raises(ValueError, match="documents"):
        metrics.dss(np.full((1, 4), 0.25), x)            # numpy alone would broadcast this one
    with pytest.raises(ValueError, match="words"):
        metrics.tss(x, np.full((3, 5), 0.2))
    with pytest.raises(ValueError, match="entries"):
        metrics.bhattacharyya(x, np.full((3, 5), 0.2))
    with pytest.raises(ValueError, match="2-D"):
        metrics.dss(x[0], x[0])


def test_bhattacharyya_host():
    rng = np.random.default_rng(1)
    # 4 entries: two square roots, a product and three additions per diagonal entry and the
    # row's own distance from 1 stay below 9 * 2^-53 = 1e-15
    p = rng.dirichlet([0.5] * 4, 9)
    bc = metrics.bhattacharyya(p.astype(np.float32), p.astype(np.float32))
    assert bc.dtype == np.float64 and bc.shape == (9, 9)
    bc = metrics.bhattacharyya(p, p)
    assert np.abs(np.diag(bc) - 1.0).max() <= 1e-15
    np.testing.assert_array_equal(bc, np.sqrt(p).dot(np.sqrt(p).T))
    assert metrics.tss(p, p) == pytest.approx(9.0, abs=9e-15)


def _cpu_model(K=6, V=90, n_docs=50):
    torch.manual_seed(0)
    tm = AVITM(input_size=V, n_components=K, hidden_sizes=(16, 12), batch_size=16, num_epochs=1,
               verbose=False, device="cpu", backend="torch")
    X = random_csr(n_docs, V, 12, seed=3)
    ds = BOWDataset(X, {i: f"wd{2 * i + 1}" for i in range(V)})
    tm.fit(ds)
    return tm, ds


def test_model_dss_tss_on_cpu():
    tm, ds = _cpu_model()
    rng = np.random.default_rng(2)
    tt = rng.dirichlet([0.1] * 4, len(ds))
    th = tm.get_doc_topic_distribution(ds, n_samples=5, seed=11).astype(np.float64)
    assert tm.dss(ds, tt, n_samples=5, seed=11) == _dss_formula(tt, th)
    assert tm.dss(ds, torch.from_numpy(tt), n_samples=5, seed=11, postprocess=True) == \
        _dss_formula(tt, postprocess_thetas(th))
    with pytest.raises(ValueError, match="documents"):
        tm.dss(ds, tt[:-1])

    Vg = 2 * tm.input_size + 3
    gt = rng.dirichlet([0.05] * Vg, 5)
    id2token = ds.idx2token
    cols = [int(id2token[i][2:]) for i in range(tm.input_size)]
    wd = tm.get_topic_word_distribution()
    ref = _tss_formula(metrics.betas_to_ground_truth_vocab(wd, id2token, Vg), gt)
    assert tm.tss(gt, cols) == pytest.approx(ref, abs=5 * (Vg + 4) * 2.0 ** -52)
    same = rng.dirichlet([0.05] * tm.input_size, 5)
    assert tm.tss(same) == _tss_formula(wd.astype(np.float64), same)
    with pytest.raises(ValueError, match="columns"):
        tm.tss(gt)
    with pytest.raises(ValueError, match="columns"):
        tm.tss(gt, cols[:-1])
    with pytest.raises(ValueError, match="columns"):
        tm.tss(gt, [Vg] * tm.input_size)
