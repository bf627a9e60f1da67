"""The float64 oracle of tests/oracle_walk.py against the project's own reference
(models/functional.py avitm_loss_explicit) on the CPU, the one-row batch-norm convention,
the tolerance rule's power against a leaked dead row, and the edge corpus."""
import copy

import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from gfedntm_amd.models.functional import avitm_loss_explicit
from tests.helpers import edge_csr
from tests.oracle_walk import NOISE_KEYS, Parity, check_edges, explicit_step, grad_scales, oracle64

V, K, H, C = 300, 20, (32, 24), 20


def _model(kind):
    torch.manual_seed(0)
    kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=16, verbose=False,
              backend="torch", device="cpu")
    if kind in ("combined", "zeroshot"):
        cls = CombinedTM if kind == "combined" else ZeroShotTM
        return cls(contextual_size=C, model_type="prodLDA", **kw).model
    return AVITM(model_type=kind, **kw).model


def _inputs(nb, seed=0, dtype=torch.float64):
    """A batch with an empty first row (the dead rows' stand-in) and an empty last row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(nb, V, dtype=dtype)
    for b in range(1, nb - 1):
        cols = torch.randperm(V, generator=g)[: int(torch.randint(1, 30, (1,), generator=g))]
        x[b, cols] = torch.randint(1, 5, (len(cols),), generator=g).to(dtype)
    eps = torch.randn(nb, K, generator=g, dtype=dtype)
    mask_h = (torch.rand(nb, H[-1], generator=g) > 0.2).to(dtype) * 1.25
    mask_t = (torch.rand(nb, K, generator=g) > 0.2).to(dtype) * 1.25
    xc = torch.randn(nb, C, generator=g, dtype=dtype)
    return x, eps, mask_h, mask_t, xc


def _x_enc(kind, x, xc):
    if kind == "combined":
        return lambda net: torch.cat([x, net.adapt_bert(xc)], 1)
    return xc if kind == "zeroshot" else None


@pytest.mark.parametrize("kind", ["prodLDA", "LDA", "combined", "zeroshot"])
@pytest.mark.parametrize("nb", [2, 5])
def test_oracle64_equals_functional_reference(kind, nb):
    """nb >= 2: the hand-written float64 step == avitm_loss_explicit on the same .double()
    model to 1e-12 of each tensor's scale -- loss, KL, RL, gradients, batch-norm buffers --
    on a batch whose first and last rows are empty."""
    model = _model(kind)
    x, eps, mask_h, mask_t, xc = _inputs(nb)
    assert float(x[0].sum()) == 0 and float(x[-1].sum()) == 0
    o = oracle64(model, x, eps, mask_h, mask_t, kl_weight=0.7, x_enc=_x_enc(kind, x, xc))
    ref = copy.deepcopy(model).double()
    ref.train()
    xe = _x_enc(kind, x, xc)
    loss, kl, rl = avitm_loss_explicit(ref, x, eps, mask_h, mask_t, kl_weight=0.7,
                                       x_enc=xe(ref.inf_net) if callable(xe) else xe)
    loss.backward()

    def rel(a, b, scale=None):
        scale = float(b.abs().max()) if scale is None else scale
        return float((a - b).abs().max()) / max(scale, 1e-300)

    assert rel(o["loss"], loss.detach()) <= 1e-12
    assert rel(o["kl"], kl.detach()) <= 1e-12
    assert rel(o["rl"], rl.detach()) <= 1e-12
    grads = {k: p.grad for k, p in ref.named_parameters()}
    assert set(grads) == set(o["grads"])
    scales = grad_scales(grads)
    for k in grads:
        assert rel(o["grads"][k], grads[k], scales[k]) <= 1e-12, k
    sd = ref.state_dict()
    assert len(o["buffers"]) == 9
    for k, v in o["buffers"].items():
        if "num_batches" in k:
            assert int(v) == int(sd[k]) == 1
        else:
            assert rel(v, sd[k]) <= 1e-12, k
    # the model handed in is untouched
    assert all(int(v) == 0 for k, v in model.state_dict().items() if "num_batches" in k)
    assert all(p.dtype == torch.float32 and p.grad is None for p in model.parameters())


@pytest.mark.parametrize("kind", ["prodLDA", "LDA"])
def test_oracle64_one_row_batch_convention(kind):
    """nb = 1 (F.batch_norm raises): the normalised heads are 0, the running variance takes
    the biased variance -- 0 -- so it decays by 1 - momentum, the running mean takes the row;
    the encoder's gradients vanish (batch norm of one row has no derivative)."""
    model = _model(kind)
    x, eps, mask_h, mask_t, _ = _inputs(3)
    x, eps, mask_h, mask_t = (t[1:2] for t in (x, eps, mask_h, mask_t))
    ref = copy.deepcopy(model).double()
    with pytest.raises(ValueError):
        avitm_loss_explicit(ref, x, eps, mask_h, mask_t)
    o = oracle64(model, x, eps, mask_h, mask_t)
    mom = model.inf_net.f_mu_batchnorm.momentum
    net = copy.deepcopy(model).double().inf_net
    z = net.f_mu(net.hiddens(net.activation(net.input_layer(x))) * mask_h).detach()
    b = o["buffers"]
    torch.testing.assert_close(b["inf_net.f_mu_batchnorm.running_var"],
                               torch.full((K,), 1 - mom, dtype=torch.float64), rtol=1e-14, atol=0)
    torch.testing.assert_close(b["inf_net.f_mu_batchnorm.running_mean"], mom * z[0],
                               rtol=1e-12, atol=1e-15)
    if kind == "prodLDA":      # the decoder's batch norm runs over the same single row
        torch.testing.assert_close(b["beta_batchnorm.running_var"],
                                   torch.full((V,), 1 - mom, dtype=torch.float64), rtol=1e-14, atol=0)
        # uniform word distribution: RL = -n_words log(1 / V + 1e-10)
        torch.testing.assert_close(o["rl"], -x.sum(1) * np.log(1.0 / V + 1e-10), rtol=1e-12, atol=0)
    assert float(o["grads"]["inf_net.input_layer.weight"].abs().max()) == 0.0
    assert float(o["grads"]["prior_variance"].abs().max()) > 0.0
    assert torch.isfinite(o["loss"])


def test_bound_catches_a_leaked_dead_row_and_passes_fp32():
    """The tolerance rule on the CPU: fp32 torch itself is inside its own bound by
    construction, while a step whose batch statistics saw one dead row (a copy of row 0, as
    prepare_next_batch leaves past nb) is outside it for the gradients -- an error of order
    scale / nb against a bound of order 1e-6 scale."""
    model = _model("prodLDA")
    nb = 16
    x, eps, mask_h, mask_t, _ = _inputs(nb, dtype=torch.float32)
    x[0, 3] = 2.0                    # (a non-empty stand-in: an empty one leaks less)
    o64 = oracle64(model, x, eps, mask_h, mask_t)
    o32 = explicit_step(copy.deepcopy(model), x, eps, mask_h, mask_t)
    dup = lambda t: torch.cat([t, t[:1]])      # noqa: E731
    leak = explicit_step(copy.deepcopy(model), dup(x), dup(eps), dup(mask_h), dup(mask_t))
    scales = grad_scales(o64["grads"])
    clean, leaked = Parity("fp32"), Parity("leak")
    for k in o64["grads"]:
        clean.check(0, k, o32["grads"][k], o64["grads"][k], o32["grads"][k], scale=scales[k])
        leaked.check(0, k, leak["grads"][k], o64["grads"][k], o32["grads"][k], scale=scales[k])
    assert not clean.failures
    caught = {f.split()[2].rstrip(":") for f in leaked.failures}
    assert {k for k in o64["grads"] if k not in NOISE_KEYS} <= caught, leaked.failures
    assert len(leaked.lines()) >= 4


@pytest.mark.parametrize("n_docs,B,Vc", [(37, 16, 701), (33, 16, 701), (51, 24, 701), (67, 64, 5000)])
def test_edge_csr_places_every_edge(n_docs, B, Vc):
    per_epoch = -(-n_docs // B)
    plan = BatchPlan.build(n_docs, B, per_epoch + 2, seed=0)
    s_partial = per_epoch - 1
    X, marks = edge_csr(n_docs, Vc, 40, plan, s_partial, seed=1)
    check_edges(X, marks, plan, s_partial, per_epoch + 2)
