"""The float64 walk of tests/oracle_walk.py for the fused update mode, where no gradient is
ever materialised: Adam and the FedAvg pre-scale run inside the kernels' epilogues
(csrc/gfk_common.h param_update / adam_update), one client per launch or several
(ops/engine.py BatchedSteps, grid z = client).

What a fused step leaves behind is the new moments and the new parameter, so those are what
``check_fused_step`` compares, each from the engine's own state before the step:

* the moments against ``m + (1 - b1)(g - m)`` and ``b2 v + (1 - b2) g^2`` with the float64
  oracle's gradient, under the project's rule e_kernel <= 8 e_fp32 + 4 ulp(scale)
  (docs/PARITY.md section 4.1; e_fp32 from the same formulas in fp32 on fp32 torch's gradient).
  With zero moments -- step 0 -- ``m' = (1 - b1) g``: a full-precision check of the gradient
  every epilogue consumed;
* the parameter against the float64 Adam step taken from the kernel's OWN new moments, so the
  comparison is free of the sign of a rounding-noise gradient (NOISE_KEYS) and can be held to
  a bound derived from adam_update's roundings (``param_bound``);
* loss, KL, RL and the batch-norm running statistics as ``oracle_walk.walk`` does.

The hyperparameters are the ones the kernels are handed: the fp32 fields of the engine's
descriptor (``hparams``), widened exactly to float64.  beta1 = 0.99 is 0.9900000095 there, and
1 - beta1 (the first step's bias correction) differs by 1e-6 of itself between the two: a
property of the interface, not an error of the arithmetic under test.

tests/test_fused_walk.py pins the check on the CPU (a torch stand-in passes, seven mutants of it
do not); tests/test_fused_walk_gpu.py runs the walks.
"""
import copy

import numpy as np
import torch

from tests.oracle_walk import (ULP32, Parity, _x_enc_of, explicit_step, fp32_step, grad_scales)

TINY32 = 2.0 ** -126          # smallest normal fp32: below it the hardware flushes to zero
# second-order terms of the first-order rounding count below (products of <= 8 roundings)
SECOND_ORDER = 1.0 + 2.0 ** -20
P_ULPS_REF = 1.0              # ulps (2^-23) of |ref| in the parameter bound
P_ULPS_STEP = 4.0             # ulps (2^-23) of |w u|


def adam_moments(m, v, g, p, hp):
    """torch.optim.Adam's moments in the dtype of the tensors:
    g += wd p;  m' = m + (1 - b1)(g - m);  v' = b2 v + (1 - b2) g^2."""
    dt = m.dtype
    b1, b2, wd = (torch.tensor(hp[k], dtype=dt, device=m.device) for k in ("beta1", "beta2", "weight_decay"))
    if hp["weight_decay"] != 0:
        g = g + wd * p
    return m + (1 - b1) * (g - m), b2 * v + (1 - b2) * g * g


def adam_step_size(m1, v1, t, hp):
    """float64: u = lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)."""
    m1, v1 = m1.double(), v1.double()
    bc1, bc2 = 1.0 - hp["beta1"] ** t, 1.0 - hp["beta2"] ** t
    return hp["lr"] / bc1 * m1 / (torch.sqrt(v1) / np.sqrt(bc2) + hp["eps"])


def param_bound(ref, wu):
    """The elementwise bound on |p' - ref|, ref = w (p - u), from adam_update's roundings.

    With m', v', p and the fp32 hyperparameters given exactly, the kernel computes
    (csrc/gfk_common.h adam_update, param_update; r = 2^-24, half an ulp, one rounding)

        den = fma(v_sqrt_f32(v'), ibc2, eps)    v_sqrt_f32 1 ulp = 2 r; ibc2 = (float) of a
                                                double, r; the fma's rounding, r:     4 r
        q   = v_rcp_f32(den)                    1 ulp = 2 r:                           2 r
        s   = step * m'                         step = (float) of a double, r; the
                                                product, r:                            2 r
        p1  = fma(-s, q, p)                     one rounding of the RESULT:    r |p - u|
        p'  = p1 * w                            one rounding of the result:    r |w (p - u)|

    so u carries 8 r = 4 ulp and the result 2 r = 1 ulp:
        |p' - ref| <= 1 * 2^-23 |ref| + 4 * 2^-23 |w u|     (first order).
    (A count that also charges the roundings of lr, eps and w to fp32 arrives at 2 and 8 ulp;
    they are exact here, see ``hparams``.)  Second-order terms are under 2^-20 of that; TINY32
    covers a product flushed to zero.  For lr = 2e-3 this is below 1e-9 + 1.2e-7 |ref|, against
    the rtol 1e-4 / atol 1e-5 of the gradient-mode walk.  Measured on an MI355X: 0.49 of the
    bound without the pre-scale (the one rounding of the last fma), up to 0.90 with it."""
    return SECOND_ORDER * ULP32 * (P_ULPS_REF * ref.abs() + P_ULPS_STEP * wu.abs()) + TINY32


def hparams(e):
    """The optimizer's hyperparameters as the kernels read them (fp32 descriptor fields, exact in
    float64), the pre-scale, and which names lie in the shared prefix."""
    m = e._m
    hp = {"lr": float(m.lr), "beta1": float(m.beta1), "beta2": float(m.beta2), "eps": float(m.adam_eps),
          "weight_decay": float(m.weight_decay), "w": float(m.fed_scale) if m.fed_scale_on else 1.0}
    for k, want in (("lr", e.lr), ("beta1", e.beta1), ("beta2", e.beta2), ("eps", e.eps),
                    ("weight_decay", e.weight_decay), ("w", 1.0 if e.fedavg_scale is None else e.fedavg_scale)):
        assert hp[k] == float(np.float32(want)), (k, hp[k], want)
    hp["n_shared"] = int(e.flat.n_shared)
    hp["offsets"] = {k: (s.offset, s.numel) for k, s in e.flat.slots.items()}
    return hp


def is_shared(hp, name):
    off, numel = hp["offsets"][name]
    assert off + numel <= hp["n_shared"] or off >= hp["n_shared"], f"{name} straddles n_shared"
    return off < hp["n_shared"]


def check_fused_step(rec, step, pre, post, o64, o32, hp, who=""):
    """One fused step against the oracle.  ``pre`` / ``post``: the state before and after it,
    {"params": {name: tensor}, "m": ..., "v": ... (exp_avg / exp_avg_sq by name), "buffers":
    {name: tensor} (running statistics and num_batches_tracked), "adam_t": int}; ``post`` also
    holds the step's "kl", "rl" (live rows) and "loss".  ``o64`` / ``o32``: explicit_step in
    float64 and fp32_step from ``pre``.  Records into ``rec`` (a Parity); returns the number of
    tensors compared: every parameter (both moments and the value), the three loss terms and
    every running statistic."""
    at = f"{step} ({who})" if who else step
    n = 0
    w = hp["w"]
    rec.check(at, "kl", post["kl"], o64["kl"], o32["kl"], cap=(1e-4, 1e-3))
    rec.check(at, "rl", post["rl"], o64["rl"], o32["rl"], cap=(1e-4, 1e-2))
    rec.check(at, "loss", post["loss"], o64["loss"], o32["loss"], cap=(1e-4, 1e-2))
    n += 3
    assert set(post["buffers"]) == set(pre["buffers"]) == set(o64["buffers"])
    for k, v in o64["buffers"].items():
        if "num_batches" in k:
            if not int(post["buffers"][k]) == int(pre["buffers"][k]) + 1 == int(v):
                rec.failures.append(f"step {at} {k}: {int(post['buffers'][k])} after "
                                    f"{int(pre['buffers'][k])}, oracle {int(v)}")
            continue
        wk = w if is_shared(hp, k) else 1.0
        rec.check(at, k, post["buffers"][k], wk * v, wk * o32["buffers"][k], cap=(1e-4, 1e-5))
        n += 1
    names = set(pre["params"])
    assert names == set(o64["grads"]) == set(o32["grads"]) == set(post["params"])
    for d in (pre, post):
        assert set(d["m"]) == set(d["v"]) == names
    scales = grad_scales(o64["grads"])
    t = pre["adam_t"] + 1
    b1, b2 = hp["beta1"], hp["beta2"]
    checked = set()
    for k in sorted(names):
        p, m, v = pre["params"][k], pre["m"][k], pre["v"][k]
        m64, v64 = adam_moments(m.double(), v.double(), o64["grads"][k].double(), p.double(), hp)
        m32, v32 = adam_moments(m.float(), v.float(), o32["grads"][k].float(), p.float(), hp)
        rec.check(at, f"adam m {k}", post["m"][k], m64, m32,
                  scale=max(float(m64.abs().max()), (1 - b1) * scales[k]))
        rec.check(at, f"adam v {k}", post["v"][k], v64, v32,
                  scale=max(float(v64.abs().max()), (1 - b2) * scales[k] ** 2))
        wk = w if is_shared(hp, k) else 1.0
        u = adam_step_size(post["m"][k], post["v"][k], t, hp)
        ref = wk * (p.double() - u)
        rec.check_elementwise(at, f"adam p {k}", post["params"][k], ref, param_bound(ref, wk * u))
        checked.add(k)
        n += 1
    if post["adam_t"] != t:
        rec.failures.append(f"step {at} adam_t: {post['adam_t']} after {pre['adam_t']}")
    assert checked == names
    return n


def snapshot(e, model):
    """The engine's state as check_fused_step reads it (copies)."""
    sd = model.state_dict()
    names = [k for k, _ in e.param_order]
    return {"params": {k: sd[k].detach().clone() for k in names},
            "m": {k: e.view_like(e.exp_avg, k).clone() for k in names},
            "v": {k: e.view_like(e.exp_avg_sq, k).clone() for k in names},
            "buffers": {k: v.detach().clone() for k, v in sd.items() if "running" in k or "num_batches" in k},
            "adam_t": int(e.adam_t.item())}


def walk_fused(tms, datas, plans, n_steps, case, fed_scales=None, launch=None):
    """Steps 0 .. n_steps - 1 on the engines of ``tms`` in their production update mode (Adam
    in the kernels' epilogues), every client's every step against the oracle from that
    client's own state before it.  One engine: ``e.step(s)``; several: ``launch()`` runs one
    step of all of them (a replay of a captured BatchedSteps.launch) between
    sync_step_counter and advance_host_step.  ``fed_scales``: the pre-scale each engine must
    carry (None: none).  Nothing is skipped: the number of compared tensors is asserted.
    Prints the PARITY lines; raises AssertionError listing every tensor over its bound."""
    from gfedntm_amd.ops.engine import UPDATE_FUSED
    M = len(tms)
    engines = [tm.engine for tm in tms]
    assert M == len(datas) == len(plans) and (M == 1) == (launch is None)
    fed_scales = [None] * M if fed_scales is None else list(fed_scales)
    for e, fs in zip(engines, fed_scales):
        # the large-batch plan keeps the generic optimizer for all but beta (lb_fused & 4)
        assert e.update_mode == UPDATE_FUSED or (e.large_batch and e._m.lb_fused & 4)
        assert e.fedavg_scale == fs and not e.graph_enabled
    rec = Parity(case)
    hps = [hparams(e) for e in engines]
    m64s = [copy.deepcopy(tm.model).double() for tm in tms]
    m32s = [copy.deepcopy(tm.model) for tm in tms]
    n_names = [len(e.param_order) + 3 + sum("running" in k for k in tm.model.state_dict())
               for e, tm in zip(engines, tms)]
    prev = [None] * M
    eps0 = []
    compared = 0
    try:
        for s in range(n_steps):
            # 1. every engine's state, into its float64 model and its fp32 twin
            pres = []
            for e, tm, m64, m32 in zip(engines, tms, m64s, m32s):
                pres.append(snapshot(e, tm.model))
                sd = {k: v.detach().clone() for k, v in tm.model.state_dict().items()}
                m64.load_state_dict(sd)
                m32.load_state_dict(sd)
            # 2. the step
            if launch is None:
                engines[0].step(s)
            else:
                for e in engines:
                    e.sync_step_counter(s)
                launch()
                for e in engines:
                    e.advance_host_step(s)
            torch.cuda.synchronize()
            for i, (e, tm, data, plan) in enumerate(zip(engines, tms, datas, plans)):
                who = f"client {i}" if M > 1 else ""
                # 3. the batch the device prepared for itself, and its step counter
                nb = int(e.ws["nb"].item())
                assert nb == int(plan.size[s]), (who, s, nb, int(plan.size[s]))
                assert np.array_equal(e.ws["doc"][:nb].cpu().numpy(), plan.batch(s)), (who, s)
                assert int(e.d_step.item()) == s + 1, (who, s, int(e.d_step.item()))
                # 4. the step's noise
                keep = 1.0 / (1.0 - float(tm.dropout))
                eps, mask_h, mask_t = (e.ws[k][:nb].clone() for k in ("eps", "mask_h", "mask_t"))
                for name, mk in (("mask_h", mask_h), ("mask_t", mask_t)):
                    ok = (mk == 0) | ((mk - keep).abs() <= 2e-7 * keep)
                    assert bool(ok.all()), f"{who} step {s}: {name} holds values other than 0 and 1/(1-p)"
                assert bool(torch.isfinite(eps).all())
                if prev[i] is not None:
                    for name, a, b in zip(("eps", "mask_h", "mask_t"), prev[i], (eps, mask_h, mask_t)):
                        r = min(a.shape[0], b.shape[0])
                        assert not torch.equal(a[:r], b[:r]), f"{who} step {s}: {name} repeats step {s - 1}'s"
                prev[i] = (eps, mask_h, mask_t)
                if s == 0:
                    eps0.append(eps)
                # 5. the oracle, and fp32 torch on the same inputs
                ids = torch.from_numpy(plan.batch(s).astype(np.int64)).to(data.device)
                x = data.dense_rows(ids)
                xc = data.contextual[ids] if data.contextual is not None else None
                kl_w = float(tm.weights.get("beta", 1.0))
                o64 = explicit_step(m64s[i], x, eps, mask_h, mask_t, kl_w, _x_enc_of(m64s[i], x, xc))
                o32 = fp32_step(m32s[i], x, eps, mask_h, mask_t, kl_w, _x_enc_of(m32s[i], x, xc))
                post = snapshot(e, tm.model)
                post.update(kl=e.ws["kl"][:nb].clone(), rl=e.ws["rl"][:nb].clone(),
                            loss=e.loss_hist[s].clone())
                n = check_fused_step(rec, s, pres[i], post, o64, o32, hps[i], who=who)
                assert n == n_names[i], (who, s, n, n_names[i])
                compared += n
        # the clients of one launch draw their own noise
        for i in range(1, M):
            r = min(eps0[0].shape[0], eps0[i].shape[0])
            assert not torch.equal(eps0[0][:r], eps0[i][:r]), f"client {i} drew client 0's eps at step 0"
        assert compared == n_steps * sum(n_names), (compared, n_steps, n_names)
        print(f"PARITY {case} | compared {compared} tensors = {n_steps} steps x {M} clients x {n_names[0]}")
    finally:
        for line in rec.lines() + rec.failures:
            print(line)
    assert not rec.failures, "\n".join(rec.failures)
    return rec
