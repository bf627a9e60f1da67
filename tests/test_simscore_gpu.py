"""Device TSS / DSS (csrc/simscore.hip) against the numpy formulas on float64 casts.

Inputs are distributions (rows summing to <= 1): ``theta_true`` ~ Dirichlet(0.1), ``theta`` ~
Dirichlet(0.1) with entries < 3e-3 zeroed and the rows renormalised, so exact zeros occur.
Every entry of either product is then <= 1 (Cauchy-Schwarz), and the tolerances are worst-case
rounding bounds of a K-term float64 dot product on both sides plus the reordered sums, not
tuned figures:

    DSS        D (Ka + Kb + 4) 2^-52 + D^2 2^-52 ref
    BC entry   (L + 4) 2^-52
    TSS        N (L + 4) 2^-52

A wrong tile weight or tail is an error of order ref / D, far outside them.
"""
import functools

import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BOWDataset
from gfedntm_amd.eval import metrics
from gfedntm_amd.ops import simscore

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DSS_SHAPES = [(1, 5, 7), (63, 5, 7), (64, 50, 50), (65, 130, 20), (130, 512, 3), (1000, 50, 50)]
BC_ROWS = [(5, 7), (50, 50), (65, 3)]
BC_LENS = [1, 63, 700, 4466, 8200]


def _dss_formula(a, b, n_docs=None):
    n_docs = len(a) if n_docs is None else n_docs
    sa = np.sqrt(a).dot(np.sqrt(a.T))
    sb = np.sqrt(b).dot(np.sqrt(b.T))
    return float(np.sum(np.abs(sa - sb)) / n_docs)


def _tss_formula(betas, topic_vectors):
    return float(np.sum(np.max(np.sqrt(betas).dot(np.sqrt(topic_vectors.T)), axis=0)))


def _dss_bound(D, Ka, Kb, ref):
    return D * (Ka + Kb + 4) * EPS + D * D * EPS * ref


def _thinned(rng, K, D):
    t = rng.dirichlet([0.1] * K, D)
    t[t < 3e-3] = 0.0
    return t / t.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _dss_case(D, Ka, Kb):
    """(theta_true, theta) on the host and the device, and the oracle's DSS."""
    rng = np.random.default_rng(1000 * D + Ka)
    a, b = rng.dirichlet([0.1] * Ka, D), _thinned(rng, Kb, D)
    assert (b == 0).any()
    for x in (a, b):
        x.setflags(write=False)
    return a, b, torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda"), _dss_formula(a, b)


@functools.lru_cache(maxsize=None)
def _bc_case(M, N, L):
    """Learned rows x [M, L] (one of them all zero) and ground-truth rows y [N, L], both zero
    on the columns a re-indexing onto a larger vocabulary leaves empty; the oracle's matrix."""
    rng = np.random.default_rng(100 * M + L)
    x, y = rng.dirichlet([0.05] * L, M), rng.dirichlet([0.05] * L, N)
    if L >= 8:
        dead = rng.choice(L, L // 8, replace=False)
        x[:, dead] = 0.0
        y[:, dead[: len(dead) // 2]] = 0.0
        x /= x.sum(1, keepdims=True)
        y /= y.sum(1, keepdims=True)
    if M > 1:
        x[M // 2] = 0.0
    for t in (x, y):
        t.setflags(write=False)
    return x, y, torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda"), \
        np.sqrt(x).dot(np.sqrt(y).T)


@pytest.mark.parametrize("D,Ka,Kb", DSS_SHAPES)
def test_dss_matches_formula(D, Ka, Kb):
    a, b, da, db, ref = _dss_case(D, Ka, Kb)
    got = simscore.dss(da, db)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
    got = float(got)
    print(f"D={D} Ka={Ka} Kb={Kb}: device {got!r} numpy {ref!r} diff {abs(got - ref):.3e} "
          f"bound {_dss_bound(D, Ka, Kb, ref):.3e}")
    assert abs(got - ref) <= _dss_bound(D, Ka, Kb, ref)
    assert metrics.dss(da, db) == got                      # CUDA tensors: the kernels
    assert metrics.dss(a, b, engine="device") == got       # numpy inputs are uploaded
    assert float(simscore.dss(da, da)) == 0.0 and float(simscore.dss(db, db)) == 0.0
    assert float(simscore.dss(db, da)) == got              # |Sa - Sb| = |Sb - Sa|, bit for bit
    # the divisor
    assert abs(float(simscore.dss(da, db, n_docs=7)) - ref * D / 7) <= \
        _dss_bound(D, Ka, Kb, ref) * D / 7


@pytest.mark.parametrize("D,Ka,Kb", [(65, 130, 20), (130, 512, 3)])
def test_dss_input_types_and_layouts(D, Ka, Kb):
    _, _, da, db, _ = _dss_case(D, Ka, Kb)
    a32, b32 = da.float(), db.float()
    want = float(simscore.dss(a32.double(), b32.double()))
    assert float(simscore.dss(a32, b32)) == want           # widening fp32 is exact
    assert float(simscore.dss(a32, b32.double())) == want
    at = da.t().contiguous().t()                           # [D, Ka] with strides (1, D)
    assert not at.is_contiguous()
    assert float(simscore.dss(at, db)) == float(simscore.dss(da, db))
    wide = torch.zeros(D, Kb + 5, dtype=torch.float64, device="cuda")
    wide[:, :Kb] = db                                      # a row stride above K
    assert float(simscore.dss(da, wide[:, :Kb])) == float(simscore.dss(da, db))


def test_dss_edges_and_validation():
    e = torch.zeros(0, 5, device="cuda")
    out = simscore.dss(e, e.double())
    assert out.dtype == torch.float64 and float(out) == 0.0
    x = torch.full((4, 5), 0.2, device="cuda")
    with pytest.raises(ValueError, match="documents"):
        simscore.dss(x, x[:3])
    with pytest.raises(ValueError, match="topics"):
        simscore.dss(x, torch.zeros(4, 513, device="cuda"))
    with pytest.raises(ValueError, match="max_grid"):
        simscore.dss(x, x, max_grid=0)
    with pytest.raises(TypeError, match="CUDA"):
        simscore.dss(x.cpu(), x)
    with pytest.raises(ValueError, match="entries"):
        simscore.bhattacharyya(x, torch.zeros(4, 6, device="cuda"))
    with pytest.raises(ValueError, match="at most"):
        simscore.bhattacharyya(torch.zeros(513, 5, device="cuda"), x)


def test_sqrt_is_correctly_rounded():
    """x against the single entry 1: the product is sqrt(x) * 1 + 0, exact after the square
    root, which must be numpy's correctly rounded one whatever the build's fast-math flags."""
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(300), 10.0 ** rng.uniform(-300, 300, 200), [0.0, 1e-310, 2.0, 4.0]])
    got = simscore.bhattacharyya(torch.from_numpy(x[:, None]).cuda(),
                                 torch.ones(1, 1, dtype=torch.float64, device="cuda"))
    np.testing.assert_array_equal(got.cpu().numpy()[:, 0], np.sqrt(x))


@pytest.mark.parametrize("L", BC_LENS)
@pytest.mark.parametrize("M,N", BC_ROWS)
def test_bc_and_tss_match_formula(M, N, L):
    x, y, dx, dy, ref = _bc_case(M, N, L)
    got = simscore.bhattacharyya(dx, dy)
    assert got.dtype == torch.float64 and tuple(got.shape) == (M, N)
    g = got.cpu().numpy()
    print(f"M={M} N={N} L={L}: BC max diff {np.abs(g - ref).max():.3e} bound {(L + 4) * EPS:.3e}")
    assert np.abs(g - ref).max() <= (L + 4) * EPS
    if M > 1:
        assert (g[M // 2] == 0.0).all()                    # the all-zero row
    t = float(simscore.tss(dx, dy))
    tref = _tss_formula(x, y)
    print(f"  TSS device {t!r} numpy {tref!r} diff {abs(t - tref):.3e} bound {N * (L + 4) * EPS:.3e}")
    assert abs(t - tref) <= N * (L + 4) * EPS
    assert metrics.tss(dx, dy) == t and metrics.tss(x, y, engine="device") == t
    assert torch.equal(metrics.bhattacharyya(dx, dy), got)
    # a set of topics against itself: every topic finds itself, BC = its own sum = 1
    assert abs(float(simscore.tss(dy, dy)) - N) <= N * (L + 4) * EPS
    # fp32 operands are widened exactly
    x32 = dx.float()
    assert torch.equal(simscore.bhattacharyya(x32, dy), simscore.bhattacharyya(x32.double(), dy))


@pytest.mark.parametrize("max_grid", [1, 3])
def test_results_do_not_depend_on_the_grid(max_grid):
    for shape in [(130, 512, 3), (1000, 50, 50)]:
        _, _, da, db, _ = _dss_case(*shape)
        assert float(simscore.dss(da, db, max_grid=max_grid)) == float(simscore.dss(da, db))
    for M, N in BC_ROWS:
        _, _, dx, dy, _ = _bc_case(M, N, 8200)
        assert torch.equal(simscore.bhattacharyya(dx, dy, max_grid=max_grid),
                           simscore.bhattacharyya(dx, dy))
        assert float(simscore.tss(dx, dy, max_grid=max_grid)) == float(simscore.tss(dx, dy))


def test_model_dss_tss_on_the_fused_engine():
    """tm.dss / tm.tss of a fused AVITM (K = 20, V = 700, 300 documents).  The thetas DSS is
    taken on never leave the device, so the host side of each comparison downloads the same
    thetas: get_doc_topic_distribution's, and for ``postprocess`` the inference kernel's fused
    threshold + L1 output (the host's float64 postprocess_thetas of the raw thetas differs
    from that fp32 kernel in the 6th digit, which is not what this test is about)."""
    from tests.test_theta_infer import _trained
    tm, X, data = _trained()
    D, V, Kt, Vg, seed = X.shape[0], X.shape[1], 12, 1000, 5
    rng = np.random.default_rng(3)
    cols = np.sort(rng.choice(Vg, V, replace=False))
    id2token = {i: f"wd{int(c)}" for i, c in enumerate(cols)}
    ds = BOWDataset(X, id2token)
    tt = rng.dirichlet([0.1] * Kt, D)

    th = tm.get_doc_topic_distribution(ds, seed=seed).astype(np.float64)
    ref = _dss_formula(tt, th)
    got = tm.dss(ds, tt, seed=seed)
    print(f"dss: device {got!r} host {ref!r}")
    assert abs(got - ref) <= _dss_bound(D, Kt, 20, ref)
    thp = tm.engine.theta_infer(tm.device_data(ds), 20, seed=seed, postprocess=True)
    thp = thp.cpu().numpy().astype(np.float64)
    refp = _dss_formula(tt, thp)
    gotp = tm.dss(ds, tt, seed=seed, postprocess=True)
    print(f"dss, postprocess: device {gotp!r} host {refp!r}")
    assert abs(gotp - refp) <= _dss_bound(D, Kt, 20, refp)

    tv = rng.dirichlet([0.05] * Vg, Kt)
    reft = _tss_formula(metrics.betas_to_ground_truth_vocab(tm.get_topic_word_distribution(),
                                                            id2token, Vg), tv)
    gott = tm.tss(tv, cols)
    print(f"tss: device {gott!r} host {reft!r}")
    assert abs(gott - reft) <= Kt * (Vg + 4) * EPS


def test_experiment_driver_metrics_engine():
    """One dss_tss iteration with "metrics_engine": "device" against "host" (same seed, same
    CPU training).  The host side computes DSS in float32, the dtype of the model's thetas,
    hence rtol 1e-5 and not a rounding bound."""
    from gfedntm_amd.experiments import dss_tss
    cfg = dict(dss_tss.DEFAULTS)
    cfg.update(n_nodes=2, vocab_size=150, n_topics=5, beta=0.05, alpha=0.5, n_docs=60,
               n_docs_inf=20, n_docs_global_inf=20, nwords=(20, 40), hidden_sizes=[16, 16],
               num_epochs=2, batch_size=16, device="cpu", backend="torch", arms=["centralized"])
    res = {}
    for engine in ("host", "device"):
        res[engine] = dss_tss.run_iteration(dict(cfg, metrics_engine=engine), 1, 0.05, "cpu",
                                            seed=0)["centralized"]
        print(engine, res[engine])
    np.testing.assert_allclose(res["device"], res["host"], rtol=1e-5)
