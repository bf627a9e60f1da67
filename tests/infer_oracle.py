"""float64 numpy oracle of the eval-mode encoder and of theta inference, written out from a
model's ``state_dict`` (shared by tests/score_oracle.py, tests/test_infer_oracle.py and the
GPU tests of csrc/infer.hip; not a test module), with the numpy twin of the kernels' Philox
draws.

Eval mode throughout: batch-norm with running statistics, no dropout.  The activations are
torch's eval-mode definitions: softplus is the identity above its threshold of 20 (as
``nn.Softplus`` and csrc/gfk_common.h act_f), RReLU uses the mean slope (1/8 + 1/3) / 2,
SELU torch's constants.  tests/test_infer_oracle.py pins ``oracle_moments`` to
``tm.model.inf_net`` in ``.double()`` on the CPU.
"""
import numpy as np
import torch

U32 = np.uint64(0xFFFFFFFF)
ULP32 = 2.0 ** -23
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934, 1.6732632423543772848
RRELU_SLOPE = (1.0 / 8.0 + 1.0 / 3.0) / 2.0


def np_state(tm):
    return {k: v.detach().double().cpu().numpy() for k, v in tm.model.state_dict().items()}


def perturb_state(tm, seed=0, gain=1.5):
    """Load a state no initialisation gives into ``tm.model`` (no training): every weight
    matrix times ``gain``, biases ~ N(0, 0.1), batch-norm running means ~ N(0, 1) and running
    variances ~ U(0.3, 3).  With ``tests/helpers.row_edge_csr`` (a count of 1000) the first
    layer's pre-activations then reach past 20 and below -5 (asserted by the callers on the
    oracle)."""
    g = torch.Generator().manual_seed(seed)
    new = {}
    for k, v in tm.model.state_dict().items():
        t = v.detach().cpu().clone()
        if not t.is_floating_point():
            pass
        elif k.endswith("running_mean"):
            t = torch.randn(t.shape, generator=g)
        elif k.endswith("running_var"):
            t = 0.3 + 2.7 * torch.rand(t.shape, generator=g)
        elif k.endswith(".bias"):
            t = 0.1 * torch.randn(t.shape, generator=g)
        elif k.endswith(".weight"):
            t = t * gain
        new[k] = t.to(v.device)
    tm.model.load_state_dict(new)
    return tm


def edge_context(n_docs, C, L, marks, seed=2):
    """(contextual embeddings [n, C] ~ N(0, 1), one-hot labels [n, L]) for the documents of
    ``row_edge_csr``; the ``count1000`` document's embedding is 40 times as long, so a
    ZeroShotTM encoder -- which never sees the counts -- meets large pre-activations too."""
    rng = np.random.default_rng(seed)
    ctx = rng.standard_normal((n_docs, C)).astype(np.float32)
    ctx[marks["count1000"]] *= 40.0
    lab = np.eye(L, dtype=np.float32)[rng.integers(0, L, n_docs)]
    return ctx, lab


def activation(name, z):
    """Eval-mode activation ``name`` (models/networks.py ACTIVATIONS) of a float64 array."""
    neg = np.minimum(z, 0.0)                 # (expm1 only ever sees the negative side)
    if name == "softplus":
        return np.where(z > 20.0, z, np.logaddexp(0.0, np.minimum(z, 20.0)))
    if name == "relu":
        return np.maximum(z, 0.0)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if name == "tanh":
        return np.tanh(z)
    if name == "leakyrelu":
        return np.where(z > 0, z, 0.01 * z)
    if name == "rrelu":
        return np.where(z >= 0, z, RRELU_SLOPE * z)
    if name == "elu":
        return np.where(z > 0, z, np.expm1(neg))
    if name == "selu":
        return SELU_SCALE * np.where(z > 0, z, SELU_ALPHA * np.expm1(neg))
    raise ValueError(f"unknown activation {name!r}")


def encoder_input(tm, X, ctx=None, labels=None, sd=None):
    """The dense float64 input of ``inf_net.input_layer``: the bag of words (AVITM); [bag of
    words | adapt_bert(ctx) | labels] (CombinedTM); [ctx | labels] (ZeroShotTM)."""
    sd = np_state(tm) if sd is None else sd
    x = np.asarray(X.toarray() if hasattr(X, "toarray") else X, dtype=np.float64)
    if tm.kind != "ctm":
        return x
    c = np.asarray(ctx, dtype=np.float64)
    if tm.inference_type == "combined":
        parts = [x, c @ sd["inf_net.adapt_bert.weight"].T + sd["inf_net.adapt_bert.bias"]]
    else:
        parts = [c]
    if labels is not None:
        parts.append(np.asarray(labels, dtype=np.float64))
    return np.concatenate(parts, 1)


def oracle_moments(tm, X, ctx=None, labels=None, return_pre=False):
    """(mu, log sigma^2) [D, K] of the eval-mode encoder: any of the eight activations, any
    number of hidden layers (``hidden_sizes`` of length 1: none), AVITM / CombinedTM /
    ZeroShotTM with or without label inputs.  ``return_pre``: also the list of every layer's
    pre-activations (input layer first)."""
    sd = np_state(tm)
    act = tm.activation
    bn_eps = tm.model.inf_net.f_mu_batchnorm.eps
    x = encoder_input(tm, X, ctx, labels, sd)
    pre = [x @ sd["inf_net.input_layer.weight"].T + sd["inf_net.input_layer.bias"]]
    h = activation(act, pre[-1])
    for l in range(len(tm.hidden_sizes) - 1):
        pre.append(h @ sd[f"inf_net.hiddens.l_{l}.0.weight"].T + sd[f"inf_net.hiddens.l_{l}.0.bias"])
        h = activation(act, pre[-1])

    def head(name):
        z = h @ sd[f"inf_net.{name}.weight"].T + sd[f"inf_net.{name}.bias"]
        return (z - sd[f"inf_net.{name}_batchnorm.running_mean"]) / np.sqrt(
            sd[f"inf_net.{name}_batchnorm.running_var"] + bn_eps)

    out = (head("f_mu"), head("f_sigma"))
    return out + (pre,) if return_pre else out


def postprocess(theta, threshold):
    """eval/export.py postprocess_thetas, restated: entries under the threshold to zero, rows
    L1-normalised, an all-zero row left as it is."""
    t = np.where(theta < threshold, 0.0, theta)
    s = t.sum(-1, keepdims=True)
    return t / np.where(s == 0, 1.0, s)


def oracle_theta(mu, ls, eps, threshold=None, dtype=np.float64):
    """mean over the S draws of softmax(mu + eps_s exp(log sigma^2 / 2)) [D, K]; ``eps``
    [S, D, K].  With a ``threshold`` the theta post-processing on top.  ``dtype=np.float32``
    restates the same formula in fp32 arithmetic (the measure of fp32's own error)."""
    mu, ls, eps = (np.asarray(a, dtype=dtype) for a in (mu, ls, eps))
    half = dtype(0.5)
    z = mu[None] + eps * np.exp(half * ls)[None]
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    th = (e / e.sum(-1, keepdims=True, dtype=dtype)).sum(0, dtype=dtype) / dtype(eps.shape[0])
    assert th.dtype == dtype
    return th if threshold is None else postprocess(th, dtype(threshold))


# ------------------------------------------------------------------ the kernels' draws
def philox4x32_10(seed: int, c0, c1, c2, c3):
    """csrc/gfk_common.h philox(): 10 rounds, key (seed lo, seed hi)."""
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    shape = np.broadcast(np.asarray(c0), np.asarray(c1), np.asarray(c2), np.asarray(c3)).shape
    x = [np.broadcast_to(np.asarray(v, dtype=np.uint64), shape).copy() for v in (c0, c1, c2, c3)]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * x[0]
        p1 = np.uint64(0xCD9E8D57) * x[2]
        x = [((p1 >> np.uint64(32)) ^ x[1] ^ k0) & U32, p1 & U32,
             ((p0 >> np.uint64(32)) ^ x[3] ^ k1) & U32, p0 & U32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return x


def infer_normals(seed: int, n_docs: int, K: int, S: int, dtype=np.float64) -> np.ndarray:
    """[S, n_docs, K] draws of csrc/infer.hip: Philox(idx = d K + k, ctr = s / 4,
    tag RNG_INFER = 4), Box-Muller on both halves.  ``dtype=np.float32``: the Box-Muller
    arithmetic of randn4 in fp32 from the same Philox integers (the uniforms are exact in
    either type)."""
    idx = (np.arange(n_docs, dtype=np.uint64)[:, None] * np.uint64(K)
           + np.arange(K, dtype=np.uint64)[None, :])
    out = np.empty((S, n_docs, K), dtype=dtype)
    two, two_pi, inv = dtype(2.0), dtype(2.0 * np.pi), dtype(1.0 / 2**24)
    for c in range((S + 3) // 4):
        r = philox4x32_10(seed, idx, c, 4, 0x5EED)
        f = [np.floor(v.astype(np.float64) / 256).astype(dtype) for v in r]     # 24 bits: exact
        u1, u2, u3, u4 = (f[0] + dtype(1)) * inv, f[1] * inv, (f[2] + dtype(1)) * inv, f[3] * inv
        ra, rb = np.sqrt(-two * np.log(u1)), np.sqrt(-two * np.log(u3))
        n4 = (ra * np.cos(two_pi * u2), ra * np.sin(two_pi * u2),
              rb * np.cos(two_pi * u4), rb * np.sin(two_pi * u4))
        for j in range(4):
            if 4 * c + j < S:
                assert n4[j].dtype == dtype
                out[4 * c + j] = n4[j]
    return out


# ------------------------------------------------------------------ the bound
def parity(kernel, f64, f32, rows=None, cap=None, factor=8.0, floor_ulps=4.0):
    """docs/PARITY.md section 4.1 on one tensor (optionally its ``rows`` alone):
    e_kernel <= 8 e_fp32 + 4 * 2^-23 * scale with scale = max |f64|, and elementwise nowhere
    looser than ``cap`` = (rtol, atol).  Returns a dict: e_kernel, e_fp32, scale, bound,
    ratio (e_kernel / e_fp32, inf when fp32 is exact and the kernel is not), use
    (e_kernel / bound), ok."""
    sel = slice(None) if rows is None else rows
    k, r64, r32 = (np.asarray(a, dtype=np.float64)[sel] for a in (kernel, f64, f32))
    err = np.abs(k - r64)
    e_k, e_32 = float(err.max()), float(np.abs(r32 - r64).max())
    scale = float(np.abs(r64).max())
    bound = factor * e_32 + floor_ulps * ULP32 * scale
    ok = bool(np.isfinite(k).all()) and e_k <= bound
    if cap is not None:
        ok = ok and bool((err <= cap[1] + cap[0] * np.abs(r64)).all())
    return {"e_kernel": e_k, "e_fp32": e_32, "scale": scale, "bound": bound,
            "ratio": e_k / e_32 if e_32 > 0 else (0.0 if e_k == 0 else float("inf")),
            "use": e_k / bound if bound > 0 else (0.0 if e_k == 0 else float("inf")), "ok": ok}
