"""The float64 oracle of tests/infer_oracle.py against the project's own encoder
(``tm.model.inf_net`` in eval mode, ``.double()``) on the CPU, the theta formula against
torch and eval/export.py, the fp32 twin of the draws, and the row-edge corpus."""
import copy

import numpy as np
import pytest
import torch

from gfedntm_amd.eval.export import postprocess_thetas
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from gfedntm_amd.models.networks import ACTIVATIONS
from gfedntm_amd.ops import kernel_abi as abi
from tests.helpers import ROW_EDGE_NNZ, row_edge_csr
from tests.infer_oracle import (edge_context, infer_normals, oracle_moments, oracle_theta, parity, perturb_state,
                                philox4x32_10)

V, K, C, L = 701, 20, 20, 5
_X, _MARKS = row_edge_csr(V, seed=1)
_CTX, _LAB = edge_context(_X.shape[0], C, L, _MARKS)


def _model(kind, H=(32, 24), activation="softplus", label_size=0):
    torch.manual_seed(0)
    kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=16, verbose=False,
              backend="torch", device="cpu", activation=activation)
    if kind in ("combined", "zeroshot"):
        cls = CombinedTM if kind == "combined" else ZeroShotTM
        tm = cls(contextual_size=C, model_type="prodLDA", label_size=label_size, **kw)
    else:
        tm = AVITM(model_type=kind, **kw)
    return perturb_state(tm, seed=3)


def _pin(tm, ctx=None, labels=None):
    """oracle_moments == inf_net.double() in eval mode, to 1e-12 of each tensor's scale; the
    pre-activations reach both softplus branches and the negative arms."""
    mu, ls, pre = oracle_moments(tm, _X, ctx, labels, return_pre=True)
    assert len(pre) == len(tm.hidden_sizes)
    assert pre[0].max() > 20.0 and pre[0].min() < -5.0
    net = copy.deepcopy(tm.model.inf_net).double().eval()
    x = torch.from_numpy(_X.toarray()).double()
    args = (x,) if tm.kind != "ctm" else (
        x, torch.from_numpy(ctx).double(), None if labels is None else torch.from_numpy(labels).double())
    with torch.no_grad():
        rmu, rls = net(*args)
    for got, ref in ((mu, rmu.numpy()), (ls, rls.numpy())):
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert all(p.dtype == torch.float32 for p in tm.model.parameters())     # untouched


@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_every_activation(activation):
    assert len(ACTIVATIONS) == 8
    _pin(_model("prodLDA", activation=activation))


@pytest.mark.parametrize("H", [(100,), (16,) * abi.MAX_LAYERS, (200, 64)])
def test_depths(H):
    """No hidden layer, the most the engine takes, two."""
    _pin(_model("prodLDA", H=H))


def test_neurallda():
    _pin(_model("LDA"))


@pytest.mark.parametrize("kind", ["combined", "zeroshot"])
@pytest.mark.parametrize("labels", [False, True])
def test_ctm_inputs(kind, labels):
    tm = _model(kind, label_size=L if labels else 0)
    _pin(tm, _CTX, _LAB if labels else None)


def test_oracle_theta_and_postprocess():
    rng = np.random.default_rng(0)
    mu, ls = rng.standard_normal((40, K)), 0.5 * rng.standard_normal((40, K))
    mu[7], ls[7] = 0.0, -40.0                   # a uniform row: 1 / K everywhere
    eps = rng.standard_normal((5, 40, K))
    th = oracle_theta(mu, ls, eps)
    ref = torch.softmax(torch.from_numpy(mu)[None] + torch.from_numpy(eps)
                        * torch.exp(0.5 * torch.from_numpy(ls))[None], -1).mean(0).numpy()
    np.testing.assert_allclose(th, ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(th.sum(1), 1.0, rtol=1e-13)
    for thr in (3e-3, 0.9):
        np.testing.assert_array_equal(oracle_theta(mu, ls, eps, threshold=thr), postprocess_thetas(th, thr))
    pp = oracle_theta(mu, ls, eps, threshold=0.9)
    assert (pp[7] == 0).all() and np.isfinite(pp).all()            # all under: the row stays zero
    th32 = oracle_theta(mu, ls, eps, dtype=np.float32)
    assert th32.dtype == np.float32 and 0 < np.abs(th32 - th).max() < 1e-6


def test_draws_fp32_twin_and_parity_rule():
    seed = 0x1234_5678_9ABC
    n64 = infer_normals(seed, 30, K, 5)
    n32 = infer_normals(seed, 30, K, 5, dtype=np.float32)
    assert n64.shape == n32.shape == (5, 30, K) and n32.dtype == np.float32
    assert 0 < np.abs(n32 - n64).max() < 1e-5
    assert abs(n64.mean()) < 0.1 and abs(n64.std() - 1) < 0.1
    # the draw of one element, from its own Philox block
    r = philox4x32_10(seed, 7 * K + 3, 1, 4, 0x5EED)
    u1, u2 = ((int(r[0]) >> 8) + 1) / 2**24, (int(r[1]) >> 8) / 2**24
    assert n64[4, 7, 3] == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    # the rule: fp32 is inside its own bound; an error of 1e-3 of the scale is not; rows apart
    p = parity(n32, n64, n32)
    assert p["ok"] and p["ratio"] == 1.0 and p["use"] < 1 / 8 + 1e-9
    bad = n32.copy()
    bad[0, 0, 0] += 1e-3
    assert not parity(bad, n64, n32)["ok"]
    assert parity(bad, n64, n32, rows=np.s_[1:])["ok"]
    assert not parity(n32, n64, n32, cap=(0.0, 1e-9))["ok"]


def test_row_edge_csr():
    n = _X.shape[0]
    nnz = np.diff(_X.indptr)
    assert n % 8 and n % 64 and 150 <= n <= 170
    assert [int(nnz[_MARKS["nnz%d" % k]]) for k in ROW_EDGE_NNZ] == list(ROW_EDGE_NNZ)
    assert nnz[0] == nnz[n - 1] == nnz[_MARKS["empty_mid"]] == 0 and 0 < _MARKS["empty_mid"] < n - 1
    assert _X[_MARKS["col0"]].indices.tolist() == [0] and _X[_MARKS["col_last"]].indices.tolist() == [V - 1]
    assert _X[_MARKS["count1000"]].data.max() == 1000
    X2, m2 = row_edge_csr(V, seed=1)
    assert m2 == _MARKS and (X2 != _X).nnz == 0
    X3, _ = row_edge_csr(8200, seed=4)
    assert X3.shape[1] == 8200
