"""tests/fused_walk.py's check pinned on the CPU, so that a red GPU walk means the kernel.

A stand-in engine -- fp32 torch (avitm_loss_explicit) and the fp32 arithmetic of adam_update
(csrc/gfk_common.h) written in torch -- passes check_fused_step with every bound used below 1;
seven mutants of it, each a bug a fused epilogue or a batched launch could have, are rejected
with a failure line naming the tensor they touch.  The moment and step formulas the check uses
are torch.optim.Adam's.
"""
import copy

import numpy as np
import pytest
import torch

from gfedntm_amd.models import AVITM
from gfedntm_amd.models.engine import make_optimizer
from gfedntm_amd.models.functional import avitm_loss_explicit
from tests.fused_walk import (adam_moments, adam_step_size, check_fused_step, is_shared, param_bound)
from tests.oracle_walk import ULP32, Parity, explicit_step, fp32_step

B, V, K, H = 8, 70, 6, (10, 8)
N_DOCS = 11                              # batches of 8 and 3, then the wrap: three steps
W_IN = "inf_net.input_layer.weight"
UNSHARED = ("prior_mean", "prior_variance")      # so that w_k = 1 is exercised too
MUTANTS = {"dead_row": ("adam m beta", "inf_net.f_mu_batchnorm.running_mean", "kl"),
           "beta_last_column": ("adam m beta",),
           "win_row_dropped": ("adam m " + W_IN,),
           "bias_correction_t_plus_1": ("adam p beta", "adam p " + W_IN),
           "prescale_missing": ("adam p beta",),
           "v_with_beta1": ("adam v beta", "adam v " + W_IN),
           "running_var_biased": ("inf_net.f_mu_batchnorm.running_var",)}


def _hp(model):
    """beta1 != beta2 (else the v-with-beta1 mutant is the original); fp32-exact values, as
    the kernels' descriptor holds them."""
    f = lambda x: float(np.float32(x))  # noqa: E731
    hp = {"lr": f(2e-3), "beta1": f(0.9), "beta2": f(0.99), "eps": f(1e-8), "weight_decay": 0.0, "w": 0.75}
    keys = [k for k, v in model.state_dict().items() if v.is_floating_point()]
    shared = [k for k in keys if k not in UNSHARED]
    hp["offsets"] = {k: (32 * i, 1) for i, k in enumerate(shared + list(UNSHARED))}
    hp["n_shared"] = 32 * len(shared)
    return hp


def _model(kind):
    torch.manual_seed(0)
    tm = AVITM(input_size=V, n_components=K, hidden_sizes=H, batch_size=B, model_type=kind,
               verbose=False, backend="torch", device="cpu")
    return copy.deepcopy(tm.model).float()


def _batches(seed=0):
    """Three steps' inputs (documents, eps, mask_h, mask_t): an epoch of 11 documents, one of
    them empty, in batches of 8 and 3, then the first batch of the next epoch."""
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(N_DOCS, V)
    for d in range(N_DOCS):
        cols = torch.randperm(V, generator=g)[: int(torch.randint(1, 20, (1,), generator=g))]
        X[d, cols] = torch.randint(1, 5, (len(cols),), generator=g).float()
    X[3] = 0                                       # an empty document
    order = torch.randperm(N_DOCS, generator=g)
    out = []
    for ids in (order[:8], order[8:], torch.randperm(N_DOCS, generator=g)[:8]):
        nb = len(ids)
        out.append((X[ids], torch.randn(nb, K, generator=g),
                    (torch.rand(nb, H[-1], generator=g) > 0.2).float() * 1.25,
                    (torch.rand(nb, K, generator=g) > 0.2).float() * 1.25))
    assert [b[0].shape[0] for b in out] == [8, 3, 8]
    return out


def _state(model, st):
    sd = model.state_dict()
    names = [k for k, _ in model.named_parameters()]
    return {"params": {k: sd[k].detach().clone() for k in names},
            "m": {k: st["m"][k].clone() for k in names}, "v": {k: st["v"][k].clone() for k in names},
            "buffers": {k: v.detach().clone() for k, v in sd.items() if "running" in k or "num_batches" in k},
            "adam_t": st["adam_t"]}


def _standin_step(model, st, batch, hp, mutant=None):
    """One fused step of the stand-in, in place on ``model`` (fp32) and ``st``: the step's
    kl, rl, loss are returned.  Adam as adam_update rounds it: coefficients from double,
    every operation in fp32."""
    x, eps, mh, mt = batch
    nb = x.shape[0]
    if mutant == "dead_row":                       # row 0 repeated behind nb, and counted
        x, eps, mh, mt = (torch.cat([a, a[:1]]) for a in (x, eps, mh, mt))
    rv_pre = {k: v.clone() for k, v in model.state_dict().items() if k.endswith("running_var")}
    model.train()
    model.zero_grad()
    loss, kl, rl = avitm_loss_explicit(model, x, eps, mh, mt)
    loss.backward()
    g = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    if mutant == "beta_last_column":
        g["beta"][:, V - 1] = 0
    if mutant == "win_row_dropped":                # one word's row of the [V, H0] gradient
        g[W_IN][:, int(torch.nonzero(x.sum(0))[-1])] = 0
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)  # noqa: E731
    t = st["adam_t"] + 1
    tc = t + 1 if mutant == "bias_correction_t_plus_1" else t
    step = f32(hp["lr"] / (1.0 - hp["beta1"] ** tc))
    ibc2 = f32(1.0 / np.sqrt(1.0 - hp["beta2"] ** tc))
    b1, b2, e_ = f32(hp["beta1"]), f32(hp["beta2"]), f32(hp["eps"])
    w = f32(hp["w"])
    with torch.no_grad():
        for k, p in model.named_parameters():
            m, v = st["m"][k], st["v"][k]
            m += (1 - b1) * (g[k] - m)
            bv = b1 if mutant == "v_with_beta1" else b2
            v.copy_(bv * v + (1 - bv) * g[k] * g[k])
            den = torch.sqrt(v) * ibc2 + e_
            p -= (step * m) * (1.0 / den)
            if is_shared(hp, k) and not (mutant == "prescale_missing" and k == "beta"):
                p *= w
        for k, buf in model.state_dict().items():
            if k.startswith("inf_net") and k.endswith("running_var") and mutant == "running_var_biased":
                mom = model.inf_net.f_mu_batchnorm.momentum
                unb = (buf - (1 - mom) * rv_pre[k]) / mom
                buf.copy_((1 - mom) * rv_pre[k] + mom * unb * (nb - 1) / nb)
            if "running" in k and is_shared(hp, k):
                buf *= w
    st["adam_t"] = t
    return {"kl": kl.detach()[:nb], "rl": rl.detach()[:nb], "loss": loss.detach()}


def _run(kind, mutant=None):
    model = _model(kind)
    assert model.inf_net.f_mu_batchnorm.momentum == model.inf_net.f_sigma_batchnorm.momentum
    hp = _hp(model)
    st = {"m": {k: torch.zeros_like(p) for k, p in model.named_parameters()},
          "v": {k: torch.zeros_like(p) for k, p in model.named_parameters()}, "adam_t": 0}
    m64, m32 = copy.deepcopy(model).double(), copy.deepcopy(model)
    rec = Parity(f"{kind} {mutant}")
    n = 0
    for s, batch in enumerate(_batches()):
        pre = _state(model, st)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        m64.load_state_dict(sd)
        m32.load_state_dict(sd)
        post_terms = _standin_step(model, st, batch, hp, mutant)
        o64 = explicit_step(m64, *batch)
        o32 = fp32_step(m32, *batch)
        post = _state(model, st)
        post.update(post_terms)
        n += check_fused_step(rec, s, pre, post, o64, o32, hp, who="client 0")
    n_params = len(list(model.named_parameters()))
    assert n == 3 * (n_params + 3 + 6)
    return rec


@pytest.mark.parametrize("kind", ["prodLDA", "LDA"])
def test_standin_passes_with_every_bound_below_one(kind):
    rec = _run(kind)
    assert not rec.failures, "\n".join(rec.failures)
    classes = set(rec.worst)
    assert {"adam m", "adam v", "adam p", "kl", "rl", "loss", "bn heads", "bn beta"} <= classes
    for c, w in rec.worst.items():
        assert w["use"] < 1.0, (c, w)
    assert rec.worst["adam p"]["use"] > 0.0       # the parameters were compared, not skipped


@pytest.mark.parametrize("kind", ["prodLDA", "LDA"])
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_rejected(kind, mutant):
    rec = _run(kind, mutant)
    for tensor in MUTANTS[mutant]:
        hits = [f for f in rec.failures if f.split(": ")[0].endswith(" " + tensor)]
        assert hits, f"{mutant}: no failure names {tensor!r}\n" + "\n".join(rec.failures)
        assert all("(client 0)" in f for f in hits)


def test_parameter_bound_is_tight():
    """One ulp of the step is inside the bound, eight are not: the bound is of the order it
    is derived at, and far below the gradient-mode walk's rtol 1e-4 / atol 1e-5."""
    p = torch.tensor([0.5, -0.03, 0.0], dtype=torch.float64)
    u = torch.tensor([2e-3, -2e-3, 1e-3], dtype=torch.float64)
    ref = 0.75 * (p - u)
    bound = param_bound(ref, 0.75 * u)
    assert bool((bound < (1e-5 + 1e-4 * ref.abs()) / 100).all())
    rec = Parity("bound")
    rec.check_elementwise(0, "adam p x", ref + 0.9 * ULP32 * (0.75 * u).abs(), ref, bound)
    assert not rec.failures
    rec.check_elementwise(0, "adam p x", ref + ULP32 * ref.abs() + 8 * ULP32 * (0.75 * u).abs(), ref, bound)
    assert len(rec.failures) == 1 and "adam p x" in rec.failures[0]


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_formulas_are_torch_adam(wd):
    """adam_moments / adam_step_size in float64 == torch.optim.Adam from make_optimizer,
    three steps, with and without weight decay."""
    g_ = torch.Generator().manual_seed(1)
    lr, beta1 = 2e-3, 0.9
    p = torch.nn.Parameter(torch.randn(5, 7, generator=g_, dtype=torch.float64))
    opt = make_optimizer([p], "adam", lr, beta1)
    opt.param_groups[0]["weight_decay"] = wd
    pg = opt.param_groups[0]
    hp = {"lr": pg["lr"], "beta1": pg["betas"][0], "beta2": pg["betas"][1], "eps": pg["eps"],
          "weight_decay": wd}
    assert (hp["beta1"], hp["beta2"]) == (beta1, 0.99)
    m, v = torch.zeros_like(p.data), torch.zeros_like(p.data)
    for t in range(1, 4):
        g = torch.randn(5, 7, generator=g_, dtype=torch.float64) * 10.0 ** (t - 2)
        before = p.detach().clone()
        p.grad = g.clone()
        opt.step()
        m, v = adam_moments(m, v, g, before, hp)
        st = opt.state[p]
        assert int(st["step"]) == t
        torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=0)
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=0)
        torch.testing.assert_close(before - adam_step_size(m, v, t, hp), p.detach(), rtol=1e-13, atol=1e-16)
