"""A float64 oracle of the training step, and a walk that checks a fused engine against it
step by step over a whole epoch (partial last batch, empty documents, the epoch wrap).

``oracle64`` restates gfedntm_amd/models/functional.py on a float64 copy of the model with
batch norm written out by hand, so it also covers a one-row batch (F.batch_norm raises there;
the engine's convention is below).  ``walk`` drives an engine in gradient mode through
``compute_grads`` / ``apply_grads`` and compares every step's loss terms, gradients, batch-norm
buffers, parameters and optimizer state with the oracle.  The bound of each comparison is
measured against the reference, not the kernel: the same step in fp32 torch (``fp32_step``:
the project's fp32 oracle avitm_loss_explicit) gives fp32's own error e_fp32 against float64,
and the kernel must stay within 8 e_fp32 + 4 ulp(scale) (docs/PARITY.md section 4.1, with the
ratios measured on the GPU).

tests/test_oracle_walk.py pins the oracle to avitm_loss_explicit on the CPU;
tests/test_epoch_walk_gpu.py runs the walks.  tests/fused_walk.py is the same walk for the fused
update mode (no gradients: the new moments and parameters) and for batched client launches.
"""
import copy
from collections import defaultdict

import numpy as np
import torch
import torch.nn.functional as F

from gfedntm_amd.models.engine import make_optimizer
from gfedntm_amd.models.functional import avitm_loss_explicit
from gfedntm_amd.models.networks import kl_terms, reconstruction_terms

# zero in exact arithmetic (tests/test_fused_kernels.py): compared at the scale of the layer
NOISE_KEYS = ("inf_net.f_mu.bias", "inf_net.f_sigma.bias", "prior_mean")
ULP32 = 2.0 ** -23


def _bn_train(z, bn):
    """Training batch norm of a BatchNorm1d(affine=False) over dim 0, by hand: the batch mean
    and biased variance normalise; the running statistics move by ``momentum``; the running
    variance is fed the unbiased variance for n > 1 rows and the biased one itself for n == 1
    -- the engine's convention (csrc/posterior.hip:155,208,1281, csrc/prodlda.hip:261,532,740,
    944,1217: ``unb = nb > 1 ? var * nb / (nb - 1) : var``; csrc/neurallda.hip:82 over K)."""
    n = z.shape[0]
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    y = (z - mean) / torch.sqrt(var + bn.eps)
    with torch.no_grad():
        unb = var * (n / (n - 1)) if n > 1 else var
        bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean)
        bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * unb)
        bn.num_batches_tracked += 1
    return y


def explicit_step(model, x, eps, mask_h, mask_t, kl_weight=1.0, x_enc=None):
    """The training step on ``model`` itself, in the model's own dtype: the forward of
    models/functional.py with the hand-written batch norm, then autograd.  ``x_enc`` is the
    encoder input when it is not the bag of words: a tensor, or a callable of the inference
    network (CombinedTM: its adapt_bert layer is part of the graph).  Updates the model's
    batch-norm buffers; returns a dict of loss, kl, rl, grads and buffers."""
    dt = next(model.parameters()).dtype
    x, eps, mask_h, mask_t = (t.to(dt) for t in (x, eps, mask_h, mask_t))
    model.train()
    model.zero_grad()
    net = model.inf_net
    x_in = x if x_enc is None else (x_enc(net) if callable(x_enc) else x_enc.to(dt))
    h = net.hiddens(net.activation(net.input_layer(x_in))) * mask_h
    mu = _bn_train(net.f_mu(h), net.f_mu_batchnorm)
    ls = _bn_train(net.f_sigma(h), net.f_sigma_batchnorm)
    theta = F.softmax(mu + eps * torch.exp(0.5 * ls), dim=1)
    thetad = theta * mask_t
    if model.is_prodlda:
        wd = F.softmax(_bn_train(thetad @ model.beta, model.beta_batchnorm), dim=1)
    else:
        wd = thetad @ F.softmax(_bn_train(model.beta, model.beta_batchnorm), dim=1)
    kl = kl_terms(model.prior_mean, model.prior_variance, mu, torch.exp(ls), ls,
                  model.n_components)
    rl = reconstruction_terms(x, wd)
    loss = (kl_weight * kl + rl).sum()
    loss.backward()
    return {"loss": loss.detach(), "kl": kl.detach(), "rl": rl.detach(),
            "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()},
            "buffers": {k: v.detach().clone() for k, v in model.state_dict().items()
                        if "running" in k or "num_batches" in k}}


def fp32_step(model, x, eps, mask_h, mask_t, kl_weight=1.0, x_enc=None):
    """fp32 torch on ``model`` (fp32), the measure of fp32's own error: the project's fp32
    oracle avitm_loss_explicit (F.batch_norm and its native backward) for two rows or more;
    one row, where F.batch_norm raises, takes the hand-written step."""
    if x.shape[0] < 2:
        return explicit_step(model, x, eps, mask_h, mask_t, kl_weight, x_enc)
    model.train()
    model.zero_grad()
    xe = x_enc(model.inf_net) if callable(x_enc) else x_enc
    loss, kl, rl = avitm_loss_explicit(model, x, eps, mask_h, mask_t, kl_weight=kl_weight, x_enc=xe)
    loss.backward()
    return {"loss": loss.detach(), "kl": kl.detach(), "rl": rl.detach(),
            "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()},
            "buffers": {k: v.detach().clone() for k, v in model.state_dict().items()
                        if "running" in k or "num_batches" in k}}


def oracle64(model, x, eps, mask_h, mask_t, kl_weight=1.0, x_enc=None):
    """The step in float64 on ``copy.deepcopy(model).double()``; ``model`` is left untouched.
    Returns loss, kl, rl, all gradients and the post-step batch-norm buffers."""
    return explicit_step(copy.deepcopy(model).double(), x, eps, mask_h, mask_t, kl_weight, x_enc)


def grad_scales(grads):
    """The scale each gradient is compared at: its own max-abs; for the NOISE_KEYS the
    largest gradient of the model (as _check_grads in tests/test_fused_kernels.py)."""
    top = max(float(g.abs().max()) for g in grads.values())
    return {k: (top if k in NOISE_KEYS else float(g.abs().max())) for k, g in grads.items()}


def tensor_class(name):
    """The row of the parity table a compared tensor belongs to."""
    if name in ("loss", "kl", "rl"):
        return name
    if name in ("thetad", "actx", "dlogit", "g", "dthetad"):   # the bf16 walk (tests/bf16_walk.py)
        return name
    for cls in ("adam m", "adam v", "adam p"):      # the fused walk (tests/fused_walk.py)
        if name.startswith(cls + " "):
            return cls
    if "running" in name:
        return "bn beta" if name.startswith("beta_batchnorm") else "bn heads"
    if name in NOISE_KEYS:
        return "grad ~0"
    for part, cls in (("adapt_bert", "grad adapt_bert"), ("input_layer", "grad W_in"),
                      ("hiddens", "grad hidden"), ("f_mu", "grad heads"), ("f_sigma", "grad heads"),
                      ("prior", "grad prior"), ("beta", "grad beta")):
        if part in name:
            return cls
    return "grad other"


class Parity:
    """Worst e_kernel / e_fp32 and worst use of the bound, per tensor class, over a walk."""
    FACTOR = 8.0
    FLOOR_ULPS = 4.0

    def __init__(self, case=""):
        self.case = case
        self.worst = defaultdict(lambda: {"ratio": 0.0, "use": 0.0, "at": ""})
        self.failures = []

    def check(self, step, name, kernel, f64, f32, scale=None, cap=None, slack=None):
        """e_kernel <= 8 e_fp32 + 4 * 2^-23 * scale, and nowhere looser than ``cap`` = (rtol,
        atol), the elementwise tolerance the fp32-oracle tests use today.  ``slack`` (default
        none): an elementwise float64 allowance added to both, derived by the caller from an
        operand it cannot observe (tests/bf16_walk.py).  Returns the bound without the slack."""
        f64 = f64.double()
        err = (kernel.double() - f64).abs()
        e_k = float(err.max())
        e_32 = float((f32.double() - f64).abs().max())
        scale = float(f64.abs().max()) if scale is None else float(scale)
        bound = self.FACTOR * e_32 + self.FLOOR_ULPS * ULP32 * scale
        if slack is not None:
            err = (err - slack.double()).clamp_min(0.0)
            e_k = float(err.max())
        over = bool((err > bound).any()) or not np.isfinite(e_k)
        if cap is not None:
            over = over or bool((err > cap[1] + cap[0] * f64.abs()).any())
        w = self.worst[tensor_class(name)]
        if e_32 > 0:
            w["ratio"] = max(w["ratio"], e_k / e_32)
        use = e_k / bound if bound > 0 else (0.0 if e_k == 0 else float("inf"))
        if use > w["use"]:
            w["use"], w["at"] = use, f"step {step} {name}"
        if over:
            self.failures.append(f"step {step} {name}: e_kernel {e_k:.3e} > bound {bound:.3e} "
                                 f"(e_fp32 {e_32:.3e}, scale {scale:.3e}, cap {cap})")
        return bound

    def check_elementwise(self, step, name, kernel, ref, bound):
        """|kernel - ref| <= bound, element by element (``bound`` a float64 tensor derived from
        the arithmetic under test: no fp32 error to measure it against, so no ratio)."""
        err = (kernel.double() - ref.double()).abs()
        use = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                          torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst = float(use.max()) if use.numel() else 0.0
        w = self.worst[tensor_class(name)]
        if worst > w["use"]:
            w["use"], w["at"] = worst, f"step {step} {name}"
        if not worst <= 1.0:
            i = int(use.flatten().argmax())
            self.failures.append(f"step {step} {name}: |kernel - ref| {float(err.flatten()[i]):.3e} > bound "
                                 f"{float(bound.flatten()[i]):.3e} at element {i} (ref "
                                 f"{float(ref.flatten()[i]):.6e}), {int((use > 1).sum())} of {use.numel()} over")

    def lines(self):
        return [f"PARITY {self.case} | {c} | e_kernel/e_fp32 {w['ratio']:.2f} | bound used {w['use']:.3f}"
                f" ({w['at']})"
                for c, w in sorted(self.worst.items())]


def _x_enc_of(model, x, xc):
    kind = getattr(model, "infnet", None)
    if kind == "combined":
        return lambda net: torch.cat([x.to(net.adapt_bert.weight.dtype),
                                      net.adapt_bert(xc.to(net.adapt_bert.weight.dtype))], 1)
    if kind == "zeroshot":
        return xc
    return None


def walk(fused_tm, data, plan, n_steps, case="", fed_scale=None):
    """Steps 0 .. n_steps - 1 of ``plan`` on ``fused_tm``'s engine (gradient mode, data
    bound), each compared with ``oracle64`` from the engine's own state before the step.
    ``fed_scale`` walks with the FedAvg pre-scale on (every float tensor of the state leaves
    the step multiplied by it: test_fedavg_prescale_covers_every_shared_tensor); the split
    step is then issued through the engine's phase interface, since compute_grads is reserved
    for gradient aggregation, which excludes the pre-scale.  Returns the Parity record; raises
    AssertionError listing every tensor over its bound."""
    from gfedntm_amd.ops import kernel_abi as abi
    from gfedntm_amd.ops.engine import UPDATE_GRAD
    e = fused_tm.engine
    assert e.update_mode == UPDATE_GRAD
    assert e.fedavg_scale == fed_scale
    w = 1.0 if fed_scale is None else float(fed_scale)
    rec = Parity(case)
    m64 = copy.deepcopy(fused_tm.model).double()
    m32 = copy.deepcopy(fused_tm.model)
    opt = make_optimizer(list(m64.parameters()), "adam", e.lr, e.beta1)
    assert opt.param_groups[0]["betas"] == (e.beta1, e.beta2)
    kl_w = float(fused_tm.weights.get("beta", 1.0))
    p_drop = float(fused_tm.dropout)
    keep = 1.0 / (1.0 - p_drop)
    prev = None
    try:
        for s in range(n_steps):
            # 1. the engine's state into the float64 model and the fp32 twin
            sd = {k: v.detach().clone() for k, v in fused_tm.model.state_dict().items()}
            m64.load_state_dict(sd)
            m32.load_state_dict(sd)
            # 2. the step without the optimizer
            if fed_scale is None:
                e.compute_grads(s)
            else:
                e.sync_step_counter(s)
                e.run_phases([p for p in e.phases() if p != abi.PH_ADAM])
                e.advance_host_step(s)
            torch.cuda.synchronize()
            # 3. the batch the device prepared for itself, and its step counter
            nb = int(e.ws["nb"].item())
            assert nb == int(plan.size[s]), (s, nb, int(plan.size[s]))
            assert np.array_equal(e.ws["doc"][:nb].cpu().numpy(), plan.batch(s)), s
            assert int(e.d_step.item()) == s + 1, (s, int(e.d_step.item()))
            # 4. the step's noise
            eps, mask_h, mask_t = (e.ws[k][:nb].clone() for k in ("eps", "mask_h", "mask_t"))
            for name, mk in (("mask_h", mask_h), ("mask_t", mask_t)):
                ok = (mk == 0) | ((mk - keep).abs() <= 2e-7 * keep)
                assert bool(ok.all()), f"step {s}: {name} holds values other than 0 and 1/(1-p)"
            assert bool(torch.isfinite(eps).all())
            if prev is not None:
                for name, a, b in zip(("eps", "mask_h", "mask_t"), prev, (eps, mask_h, mask_t)):
                    r = min(a.shape[0], b.shape[0])
                    assert not torch.equal(a[:r], b[:r]), f"step {s}: {name} repeats step {s - 1}'s"
            prev = (eps, mask_h, mask_t)
            # 5. the oracle, and fp32 torch on the same inputs
            ids = torch.from_numpy(plan.batch(s).astype(np.int64)).to(data.device)
            x = data.dense_rows(ids)
            xc = data.contextual[ids] if data.contextual is not None else None
            o64 = explicit_step(m64, x, eps, mask_h, mask_t, kl_w, _x_enc_of(m64, x, xc))
            o32 = fp32_step(m32, x, eps, mask_h, mask_t, kl_w, _x_enc_of(m32, x, xc))
            rec.check(s, "kl", e.ws["kl"][:nb], o64["kl"], o32["kl"], cap=(1e-4, 1e-3))
            rec.check(s, "rl", e.ws["rl"][:nb], o64["rl"], o32["rl"], cap=(1e-4, 1e-2))
            rec.check(s, "loss", e.loss_hist[s], o64["loss"], o32["loss"], cap=(1e-4, 1e-2))
            scales = grad_scales(o64["grads"])
            top = max(scales.values())
            g = {k: e.gradient(k).detach().clone() for k, _ in e.param_order}
            assert set(g) == set(o64["grads"])
            for k in g:
                cap = (2e-3, 1e-3 * top if k in NOISE_KEYS else 2e-4 * (scales[k] + 1e-6) + 1e-4)
                rec.check(s, k, g[k], o64["grads"][k], o32["grads"][k], scale=scales[k], cap=cap)
            sd_f = fused_tm.model.state_dict()
            for k, v in o64["buffers"].items():
                if "num_batches" in k:
                    assert int(sd_f[k]) == int(v) == s + 1, (s, k, int(sd_f[k]))
                    continue
                rec.check(s, k, sd_f[k], w * v, w * o32["buffers"][k], cap=(1e-4, 1e-5))
            # 6. the optimizer in isolation: torch Adam in float64 on the kernel's own gradients
            for k, p in m64.named_parameters():
                p.grad = g[k].double()
            opt.step()
            e.apply_grads(s)
            torch.cuda.synchronize()
            sd_f = fused_tm.model.state_dict()
            for k, p in m64.named_parameters():
                torch.testing.assert_close(sd_f[k].double(), w * p.detach(), rtol=1e-4, atol=1e-5,
                                           msg=lambda m, k=k: f"step {s} {k} after Adam: {m}")
            assert int(e.adam_t.item()) == s + 1
            # 7. the gradients are consumed
            assert float(e.grad.abs().max().item()) == 0.0
        sd_e, sd_t = e.optimizer_state_dict(), opt.state_dict()
        for i, st in sd_t["state"].items():
            assert set(sd_e["state"][i]) == set(st)
            for key, val in st.items():
                if key == "step":
                    assert float(sd_e["state"][i][key]) == float(val) == n_steps
                    continue
                atol = 1e-5 * float(val.abs().max()) + 1e-6
                torch.testing.assert_close(sd_e["state"][i][key].double(), val, rtol=1e-3, atol=atol,
                                           msg=lambda m, i=i, key=key: f"optimizer state {i}.{key}: {m}")
    finally:
        for line in rec.lines() + rec.failures:
            print(line)
    assert not rec.failures, "\n".join(rec.failures)
    return rec


def check_edges(X, marks, plan, s_partial, n_steps):
    """Host-side: each edge document has its property and is walked by steps < n_steps."""
    n_docs, Vc = X.shape
    X = X.tocsr()
    row = lambda d: (X.indices[X.indptr[d]: X.indptr[d + 1]], X.data[X.indptr[d]: X.indptr[d + 1]])  # noqa: E731
    assert marks["empty_standin"] == int(plan.batch(s_partial)[0])
    assert int(plan.size[s_partial]) == n_docs % plan.batch_size != 0
    assert marks["empty_first"] == 0 and marks["empty_last"] == n_docs - 1
    for k in ("empty_standin", "empty_first", "empty_last"):
        assert len(row(marks[k])[0]) == 0
    assert list(row(marks["col0"])[0]) == [0] and list(row(marks["col_last"])[0]) == [Vc - 1]
    n_tiles = -(-Vc // 64)
    cols, _ = row(marks["last_tile"])
    assert len(cols) > 0 and cols.min() >= 64 * (n_tiles - 1)
    assert row(marks["count1000"])[1].max() == 1000
    cols, _ = row(marks["every_tile"])
    assert sorted(set(cols // 64)) == list(range(n_tiles)) and len(cols) == n_tiles
    assert len(set(marks.values())) >= 6
    walked = set(np.concatenate([plan.batch(s) for s in range(n_steps)]).tolist())
    assert set(marks.values()) <= walked
    assert (np.diff(X.indptr) == 0).sum() >= len({marks[k] for k in marks if k.startswith("empty")})
