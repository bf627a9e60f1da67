"""The float64 walk of tests/oracle_walk.py for matmul_dtype = "bf16".

A bf16 rounding is discontinuous: a kernel value one fp32 ulp from the oracle's can round to
the neighbouring bf16 value, so an oracle run end to end from the parameters cannot be held
to fp32 accuracy.  The step is therefore split where the kernels round, and wherever the
kernel's fp32 operand of a rounded GEMM is in the workspace the oracle is fed the kernel's own
bits (teacher forcing, as the Gibbs oracle does):

1. encoder forward, float64, against ws["thetad"] (CombinedTM: A = bf(x_ctx) bf(Wa)^T + b
   against ws["actx"], then z0 with the KERNEL's A rounded);
2. decoder forward from the kernel's theta_d: bf(theta_d) bf(beta) (NeuralLDA: bf(theta_d)
   bf(beta_sm)); rl, loss and beta's batch-norm buffers;
3. decoder backward with the operands the kernels' backward uses (csrc/prodlda.hip
   prodlda_bwd_body: d theta_d = bf(dlogit) bf(beta)^T, dbeta = bf(theta_d)^T bf(dlogit);
   csrc/neurallda.hip: d theta_d = g bf(beta_sm)^T with g unrounded, G = bf(g)^T bf(theta_d),
   c_k and the softmax / batch-norm backward on unrounded values), dlogit forced from ws["dt"]
   where prodlda_dlogit stored it, g from ws["dbsm"];
4. encoder backward: autograd through the float64 encoder from ws["dtheta"], row_bwd's fp32 sum
   of the d theta_d slabs (the slabs' float64 sum is what step 3 is compared with)
   (CombinedTM: csrc/ctx.hip's backward and win_update are fp32 on the unrounded A and Wc);
5. Adam in isolation, the counters and the device-prepared batch as oracle_walk.walk.

Every comparison is the project's rule e_kernel <= 8 e_fp32 + 4 ulp(scale) (docs/PARITY.md
section 4.1), e_fp32 from fp32 torch given the same already-rounded operands (bf16 values are
exact in fp32: it measures accumulation only).  Which GEMMs round is a ``Plan``, derived by the
test from the engine (FusedEngine.gemm_dtypes).

The slack.  Where a rounded operand y is not observable (dlogit without prodlda_dlogit;
beta_sm always), an element is ambiguous if its float64 value lies within
delta = 8 e_fp32(y) + 4 * 2^-23 max|y| of a bf16 rounding boundary: either neighbour is then
admissible, and each output element is allowed an extra sum |other operand| * spacing(y) over
the ambiguous terms of its sum (``ambiguity``; for dlogit the rule is applied per vocabulary
column, each column being a batch-norm backward of its own).  ``SLACK_CAP``: in every step at
most half of the elements of dbeta and d theta_d may carry a slack above their fp32-rule bound,
asserted on the oracle alone -- a cap that keeps the slack from hiding a failure, not a
measurement.  ProdLDA's d theta_d sums V terms and would always exceed it, so dlogit's
ambiguous roundings are first resolved from the kernel's own dbeta (``resolve_rounding``); only
an unresolved column keeps the slack.  Measurements: docs/PARITY.md section 4.4.

tests/test_bf16_walk.py pins all this on the CPU (a torch stand-in passes, eight mutants do
not); tests/test_bf16_walk_gpu.py runs the walks.
"""
import copy
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from gfedntm_amd.models.engine import make_optimizer
from gfedntm_amd.models.networks import kl_terms, reconstruction_terms
from tests.oracle_walk import NOISE_KEYS, ULP32, Parity, _bn_train, grad_scales

SLACK_CAP = 0.5
RL_EPS = 1e-10
SECOND_ORDER = 1.0 + 2.0 ** -7      # the first-order slack of rl and g (relative steps of 2^-8)


# ---------------------------------------------------------------- rounding to bf16
def bf16_from_f32(t):
    """fp32 bits -> the bf16 value (as fp32), exactly as v_cvt_pk_bf16_f32 rounds: add
    0x7FFF + lsb on the integer view, drop the low 16 bits (round to nearest even; the largest
    finite fp32 values overflow to infinity, as the instruction's do)."""
    assert t.dtype == torch.float32
    i = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (((i + 0x7FFF + ((i >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return torch.where(torch.isnan(t), t, r.view(torch.float32)).view(t.shape)


def bf16_from_f64(t):
    """float64 -> the nearest bf16 value (as float64), rounded ONCE, ties to even: frexp,
    rint(m 2^8), ldexp.  (Through fp32 would round twice.)  Normal bf16 range only."""
    assert t.dtype == torch.float64
    m, e = torch.frexp(t)
    return torch.round(m * 256.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=t.device),
                                              (e - 8).double())


def bf16_trunc_f32(t):
    """Toward zero: the low 16 bits dropped (a mutant's rounding, tests/test_bf16_walk.py)."""
    i = t.contiguous().view(torch.int32)
    return (i & -65536).view(torch.float32).view(t.shape)


def bf16_spacing(y):
    """The distance between the bf16 values around y (float64; 2^-8 of y's binade top)."""
    _, e = torch.frexp(y)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=y.device), (e - 8).double())


def ambiguity(y64, y32, dim=None):
    """(term, delta): ``term`` [like y] is 0 where bf(y) is decided and otherwise the most the
    kernel's rounded y may differ from the oracle's.  delta = 8 e_fp32(y) + 4 * 2^-23 max|y|
    is what the rule allows the kernel's unrounded y; ``dim``: the rule applied to every slice
    along that dimension on its own (a tensor of deltas) where the kernel computes the slices
    independently -- never a larger delta than the whole tensor's, so never more slack.
    With u = spacing(y): an element within
    delta of a rounding boundary (a midpoint between neighbouring bf16 values; the nearest one
    across a binade's bottom lies u / 4 away) may take either neighbour: one spacing.  An
    element so small that delta >= u / 4 (it carries the floor of a much larger max|y|) may
    move by delta before the rounding and half a spacing by each rounding: u + delta.  An
    exact zero is structural (a masked row or column: zero in the kernel too)."""
    y64 = y64.double()
    err = (y32.double() - y64).abs()
    if dim is None:
        delta = Parity.FACTOR * float(err.max()) + Parity.FLOOR_ULPS * ULP32 * float(y64.abs().max())
    else:
        delta = (Parity.FACTOR * err.amax(dim, keepdim=True)
                 + Parity.FLOOR_ULPS * ULP32 * y64.abs().amax(dim, keepdim=True))
    u = bf16_spacing(y64)
    q = y64.abs() / u                                      # in [128, 256)
    dist = ((q - torch.floor(q)) - 0.5).abs() * u          # to the nearest midpoint of the binade
    dist = torch.minimum(dist, (q - 127.75) * u)           # ... or the one below the binade
    small = delta >= 0.25 * u
    term = torch.where(small, u + delta, torch.where(dist <= delta, u, torch.zeros_like(u)))
    return torch.where(y64 == 0, torch.zeros_like(u), term), delta


def resolve_rounding(yr, y, term, th_r, db_k):
    """Teacher forcing from the output.  The kernel's dbeta[:, v] = bf(theta_d)^T bf(y[:, v]) is
    K equations on column v's few ambiguous roundings, and neighbouring bf16 values move it by
    2^-8 of a term where fp32 accumulation moves it by 2^-23: it says which neighbour each one
    took.  Per column with ambiguous rows A_v (at most K / 2 of them), least squares for the
    corrections c over A_v of  db_k[:, v] - bf(theta_d)^T yr[:, v] = bf(theta_d)[A_v]^T c,
    snapped to multiples of half a spacing (the spacing halves below a binade's bottom).  A
    column is RESOLVED when every snapped correction is admissible: no larger than its
    ``term`` and, for a non-zero one, on y's side of yr.  (An element dwarfed by max|y| --
    term above its spacing -- moves dbeta by less than fp32 accumulation does: its fitted
    correction is that noise, bounded by its term and as harmless in d theta_d.)  Resolved
    columns take yr + c and carry
    no slack -- dbeta and d theta_d are then held to the plain rule there, dbeta's K values
    against |A_v| choices; the others keep yr and the slack.  Never looser than the slack
    alone, since that is what an unresolved column gets.
    yr, y, term: [nb, V] float64 (the oracle's rounded y, y, ``ambiguity``'s term);
    th_r: bf(theta_d) [nb, K]; db_k: the kernel's dbeta [K, V].  Returns (yr', unresolved
    [V] bool)."""
    nb, V = y.shape
    K = th_r.shape[1]
    amb = term > 0
    n_amb = amb.sum(0)
    # (a row whose theta_d is all zero leaves no trace in dbeta)
    unresolved = (n_amb > max(K // 2, 1)) | (amb & (th_r.abs().sum(1) == 0)[:, None]).any(0)
    cols = torch.nonzero((n_amb > 0) & ~unresolved).flatten()
    if cols.numel() == 0:
        return yr, unresolved
    A = amb[:, cols].t().double()                                   # [nc, nb]
    resid = db_k.double()[:, cols] - th_r.t() @ yr[:, cols]         # [K, nc]
    gram = th_r @ th_r.t()                                          # [nb, nb]
    ridge = 1e-12 * float(gram.diagonal().mean()) + 1e-300
    M = A[:, :, None] * gram[None] * A[:, None, :] + torch.diag_embed(1.0 - A + ridge * A)
    c = torch.linalg.solve(M, (A * (th_r @ resid).t())[:, :, None])[:, :, 0].t()   # [nb, nc]
    u = bf16_spacing(y[:, cols])
    c = torch.round(2.0 * c / u) * 0.5 * u * amb[:, cols]
    side = torch.sign(y[:, cols] - yr[:, cols])
    # (an element dwarfed by max|y| may sit on either side; a boundary one only across it)
    small = term[:, cols] > u
    ok = (c.abs() <= term[:, cols]) & ((c == 0) | small | (torch.sign(c) == side))
    good = ok.all(0)
    out = yr.clone()
    out[:, cols[good]] = yr[:, cols[good]] + c[:, good]
    unresolved[cols[~good]] = True
    return out, unresolved


# ---------------------------------------------------------------- the plan
@dataclass(frozen=True)
class Plan:
    """Which GEMMs take bf16 operands (FusedEngine.gemm_dtypes)."""
    fwd: bool = True
    dthetad: bool = True
    dbeta: bool = True
    ctx_a: bool = False
    ctx_z0: bool = False

    @classmethod
    def of(cls, gemm_dtypes):
        assert set(gemm_dtypes) == {"dec_fwd", "dthetad", "dbeta", "ctx_a", "ctx_z0"}
        assert all(v in ("bf16", "fp32", None) for v in gemm_dtypes.values())
        b = lambda k: gemm_dtypes[k] == "bf16"  # noqa: E731
        return cls(b("dec_fwd"), b("dthetad"), b("dbeta"), b("ctx_a"), b("ctx_z0"))


# ---------------------------------------------------------------- the step, piece by piece
def _bn(z, bn, native):
    """Training batch norm: by hand (float64; one row), or F.batch_norm (fp32 torch's own)."""
    if not native or z.shape[0] < 2:
        return _bn_train(z, bn)
    y = F.batch_norm(z, bn.running_mean, bn.running_var, training=True, momentum=bn.momentum, eps=bn.eps)
    bn.num_batches_tracked += 1
    return y


def _r(t, dt):
    """The bf16 rounding of a KERNEL fp32 tensor (exact from its bits), in dtype dt."""
    return bf16_from_f32(t.detach().float()).to(dt)


class _CtxMM(torch.autograd.Function):
    """A Wc^T with bf16 operands forward (the kernel's A, rounded; Wc rounded) and the kernels'
    fp32 backward on the unrounded operands: dA = g Wc, dWc = g^T A (csrc/ctx.hip ctx_bwd,
    csrc/update.hip win_tile_ctx read ws_actx and Wc as they are)."""

    @staticmethod
    def forward(ctx, a_graph, wc, a_kernel):
        dt = wc.dtype
        ctx.save_for_backward(wc, a_kernel.to(dt))
        return _r(a_kernel, dt) @ _r(wc, dt).t()

    @staticmethod
    def backward(ctx, g):
        wc, a = ctx.saved_tensors
        return g @ wc, g.t() @ a, None


def encoder(model, x, xc, eps, mask_h, mask_t, plan, native, a_kernel=None):
    """The encoder forward on ``model`` in its own dtype.  Returns theta_d, kl (both in the
    autograd graph) and, for CombinedTM, the adapted rows A as the forward GEMM computes them
    (bf(x_ctx) bf(Wa)^T + b under plan.ctx_a).  CombinedTM with plan.ctx_z0: the input layer's
    contextual term takes ``a_kernel`` (the kernel's ws["actx"] rows) rounded."""
    dt = next(model.parameters()).dtype
    x, eps, mask_h, mask_t = (t.to(dt) for t in (x, eps, mask_h, mask_t))
    net = model.inf_net
    a_val = None
    if getattr(model, "infnet", None) == "combined":
        V = x.shape[1]
        xc = xc.to(dt)
        Wa, ba = net.adapt_bert.weight, net.adapt_bert.bias
        a_graph = xc @ Wa.t() + ba
        a_val = (_r(xc, dt) @ _r(Wa, dt).t() + ba).detach() if plan.ctx_a else a_graph.detach()
        W = net.input_layer.weight
        if plan.ctx_z0:
            z0 = x @ W[:, :V].t() + _CtxMM.apply(a_graph, W[:, V:2 * V], a_kernel) + net.input_layer.bias
        else:
            z0 = net.input_layer(torch.cat([x, a_graph], 1))
    else:
        assert getattr(model, "infnet", None) in (None, "bow"), getattr(model, "infnet", None)
        z0 = net.input_layer(x)
    h = net.hiddens(net.activation(z0)) * mask_h
    mu = _bn(net.f_mu(h), net.f_mu_batchnorm, native)
    ls = _bn(net.f_sigma(h), net.f_sigma_batchnorm, native)
    thetad = F.softmax(mu + eps * torch.exp(0.5 * ls), dim=1) * mask_t
    kl = kl_terms(model.prior_mean, model.prior_variance, mu, torch.exp(ls), ls, model.n_components)
    return thetad, kl, a_val


def prodlda_forward(model, x, thd_k, plan, native):
    """logits = bf(theta_d) bf(beta) from the kernel's theta_d; returns rl and dlogit =
    d sum(rl) / d logits (before the batch norm: the tile prodlda_bwd_body's GEMMs read)."""
    dt = model.beta.dtype
    beta = model.beta.detach()
    th = thd_k.to(dt)
    z = (_r(thd_k, dt) @ _r(beta, dt) if plan.fwd else th @ beta).requires_grad_(True)
    wd = F.softmax(_bn(z, model.beta_batchnorm, native), dim=1)
    rl = reconstruction_terms(x.to(dt), wd)
    (dl,) = torch.autograd.grad(rl.sum(), z)
    return rl.detach(), dl


def prodlda_backward(model, thd_k, dl, dl_rounded, plan):
    """d theta_d and dbeta with the kernel's operands; ``dl_rounded``: bf(dlogit) in this dtype
    (from the kernel's stored tile, or the float64 oracle's own, rounded once)."""
    dt = model.beta.dtype
    beta = model.beta.detach()
    dth = dl_rounded @ _r(beta, dt).t() if plan.dthetad else dl @ beta.t()
    db = _r(thd_k, dt).t() @ dl_rounded if plan.dbeta else thd_k.to(dt).t() @ dl
    return dth, db


def lda_forward(model, x, thd_k, plan, native, bsm_rounded=None):
    """word_dist = bf(theta_d) bf(beta_sm) at the non-zeros; returns rl, g = -x / (wd + 1e-10)
    (dense, zero off the non-zeros), beta_sm (in the graph of beta) and bf(beta_sm) as used
    (``bsm_rounded``: fp32 torch is handed the oracle's)."""
    dt = model.beta.dtype
    bsm = F.softmax(_bn(model.beta, model.beta_batchnorm, native), dim=1)
    if bsm_rounded is None:
        bsm_rounded = bf16_from_f64(bsm.detach()) if dt == torch.float64 else _r(bsm, dt)
    x = x.to(dt)
    wd = (_r(thd_k, dt) @ bsm_rounded) if plan.fwd else thd_k.to(dt) @ bsm.detach()
    rl = reconstruction_terms(x, wd)
    g = torch.where(x != 0, -x / (wd + RL_EPS), torch.zeros_like(wd))
    return rl, g, wd, bsm, bsm_rounded


def _bn_backward_of(model, d, native):
    """The batch norm's backward alone: d beta for dL / d beta_bn = d, on a scratch copy of the
    batch-norm module (no second update of the running statistics)."""
    bn = copy.deepcopy(model.beta_batchnorm)
    beta = model.beta.detach().clone().requires_grad_(True)
    (db,) = torch.autograd.grad(_bn(beta, bn, native), beta, grad_outputs=d)
    return db


def lda_backward(model, thd_k, g_k, dthd_k, bsm, bsm_rounded, plan, native):
    """d theta_d = g bf(beta_sm)^T (g unrounded: the kernel's own); G = bf(g)^T bf(theta_d);
    c_k = sum_b theta_d d theta_d on the kernel's unrounded values; dbeta through the softmax
    (beta_sm (G^T - c_k), written out: autograd's would take c_k from G) and the batch norm
    over the topics, unrounded."""
    dt = model.beta.dtype
    g = g_k.to(dt)
    bsm = bsm.detach()
    dth = g @ (bsm_rounded if plan.dthetad else bsm).t()
    G = _r(g_k, dt).t() @ _r(thd_k, dt) if plan.dbeta else g.t() @ thd_k.to(dt)         # [V, K]
    ck = (thd_k.to(dt) * dthd_k.to(dt)).sum(0)
    return dth, G, _bn_backward_of(model, bsm * (G.t() - ck[:, None]), native)


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _buffers(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()
            if "running" in k or "num_batches" in k}


def check_bf16_step(rec, s, m64, m32, obs, x, xc, noise, plan, kl_w=1.0, w=1.0):
    """One step of the kernels (``obs``) against the split oracle.  ``m64`` / ``m32``: the
    float64 model and its fp32 twin holding the state BEFORE the step (their batch-norm buffers
    are advanced).  ``obs``: what the step left behind, live rows only --
    thetad [nb, K], actx [nb, V] (CombinedTM), dlogit [nb, V] or None (ProdLDA), g [nb, V]
    (NeuralLDA), dthetad [nb, K] (the slabs summed in float64), kl, rl, loss, grads {name:
    tensor}, buffers {name: tensor}; optionally dtheta [nb, K], row_bwd's fp32 sum of the slabs
    (held to the n_slab roundings of that sum, and then the operand of everything behind the
    decoder, as it is the kernels'), with dthetad_slabs = (n_slab, sum of |slab|).  ``w``: the
    FedAvg pre-scale the buffers carry.
    Returns {"dbeta": share, "dthetad": share}: the share of elements whose slack exceeds their
    fp32-rule bound (a property of the oracle alone; ``assert_cap`` holds it to SLACK_CAP)."""
    eps, mask_h, mask_t = noise
    thd_k, dthd_k = obs["thetad"], obs["dthetad"].double()
    # what the kernels after the decoder read: row_bwd's fp32 sum of the slabs (ws["dtheta"])
    dth_in = obs.get("dtheta", obs["dthetad"]).double()
    if "dtheta" in obs:
        n_slab, sum_abs = obs["dthetad_slabs"]
        rec.check_elementwise(s, "dthetad", obs["dtheta"], dthd_k, n_slab * 0.5 * ULP32 * sum_abs.double() + 1e-300)
    prod = bool(m64.is_prodlda)
    for m in (m64, m32):
        m.train()
        m.zero_grad()
    # 1. encoder forward
    a_k = obs.get("actx")
    th64, kl64, a64 = encoder(m64, x, xc, eps, mask_h, mask_t, plan, False, a_k)
    th32, kl32, a32 = encoder(m32, x, xc, eps, mask_h, mask_t, plan, True, a_k)
    if a64 is not None:
        rec.check(s, "actx", a_k, a64, a32)
    rec.check(s, "thetad", thd_k, th64.detach(), th32.detach())
    rec.check(s, "kl", obs["kl"], kl64.detach(), kl32.detach(), cap=(1e-4, 1e-3))
    # 2. + 3. the decoder from the kernel's theta_d
    slack = {"dbeta": None, "dthetad": None, "rl": None}
    if prod:
        rl64, dl64 = prodlda_forward(m64, x, thd_k, plan, False)
        rl32, dl32 = prodlda_forward(m32, x, thd_k, plan, True)
        dl_k = obs.get("dlogit")
        rounds = plan.dthetad or plan.dbeta
        if dl_k is not None:
            rec.check(s, "dlogit", dl_k, dl64, dl32)
            dlr64 = _r(dl_k, torch.float64)
            dl64 = dl_k.double()                    # (an unrounded GEMM of a mixed plan reads it too)
            dl32 = dl_k.float()
        else:
            dlr64 = bf16_from_f64(dl64)
            if rounds:
                # (a column of dlogit is one batch-norm backward of its own: 16 lanes per column
                # in prodlda_bwd_body and prodlda_dlogit, its sums over the column's rows only)
                term, _ = ambiguity(dl64, dl32, dim=0)
                if plan.dbeta:
                    dlr64, unresolved = resolve_rounding(dlr64, dl64, term, _r(thd_k, torch.float64),
                                                         obs["grads"]["beta"])
                    term = term * unresolved.double()[None, :]
                if plan.dbeta:
                    slack["dbeta"] = _r(thd_k, torch.float64).abs().t() @ term
                if plan.dthetad:
                    slack["dthetad"] = term @ _r(m64.beta.detach(), torch.float64).abs().t()
        dth64, db64 = prodlda_backward(m64, thd_k, dl64, dlr64, plan)
        dth32, db32 = prodlda_backward(m32, thd_k, dl32, dlr64.float(), plan)
    else:
        g_k = obs["g"]
        rl64, g64, wd64, bsm64, bsr64 = lda_forward(m64, x, thd_k, plan, False)
        # fp32 torch's own beta_sm measures e_fp32(beta_sm); its GEMMs take the oracle's rounding
        rl32, g32, _, bsm32, _ = lda_forward(m32, x, thd_k, plan, True, bsr64.float())
        slack_g = None
        if plan.fwd or plan.dthetad:
            term, _ = ambiguity(bsm64.detach(), bsm32.detach())          # [K, V]
            if plan.fwd:
                s_wd = _r(thd_k, torch.float64).abs() @ term
                slack_g = SECOND_ORDER * g64.abs() / (wd64 + RL_EPS) * s_wd
                slack["rl"] = SECOND_ORDER * (g64.abs() * s_wd).sum(1)
            if plan.dthetad:
                slack["dthetad"] = g_k.double().abs() @ term.t()
        rec.check(s, "g", g_k, g64, g32, slack=slack_g)
        rl64, rl32 = rl64.detach(), rl32.detach()
        dth64, G64, db64 = lda_backward(m64, thd_k, g_k, dth_in, bsm64, bsr64, plan, False)
        dth32, G32, db32 = lda_backward(m32, thd_k, g_k, dth_in, bsm32, bsr64.float(), plan, True)
    rec.check(s, "rl", obs["rl"], rl64, rl32, cap=(1e-4, 1e-2), slack=slack["rl"])
    loss64 = kl_w * kl64.detach().sum() + rl64.sum()
    loss32 = kl_w * kl32.detach().sum() + rl32.sum()
    rec.check(s, "loss", obs["loss"], loss64, loss32, cap=(1e-4, 1e-2),
              slack=None if slack["rl"] is None else slack["rl"].sum())
    b_dth = rec.check(s, "dthetad", dthd_k, dth64, dth32, slack=slack["dthetad"])
    # 4. encoder backward from the kernel's d theta_d
    (kl_w * kl64.sum() + (th64 * dth_in).sum()).backward()
    (kl_w * kl32.sum() + (th32 * dth_in.float()).sum()).backward()
    m64.beta.grad, m32.beta.grad = db64.detach(), db32.detach()
    g64s, g32s = _grads(m64), _grads(m32)
    assert set(obs["grads"]) == set(g64s)
    scales = grad_scales(g64s)
    top = max(scales.values())
    b_db = None
    for k, gk in obs["grads"].items():
        cap = (2e-3, 1e-3 * top if k in NOISE_KEYS else 2e-4 * (scales[k] + 1e-6) + 1e-4)
        sl = slack["dbeta"] if k == "beta" else None
        if sl is not None:
            cap = None              # (the fp32-oracle tolerance knows no admissible neighbour)
        b = rec.check(s, k, gk, g64s[k], g32s[k], scale=scales[k], cap=cap, slack=sl)
        if k == "beta":
            b_db = b
    b64, b32 = _buffers(m64), _buffers(m32)
    for k, v in b64.items():
        if "num_batches" in k:
            if int(obs["buffers"][k]) != int(v):
                rec.failures.append(f"step {s} {k}: {int(obs['buffers'][k])}, oracle {int(v)}")
            continue
        rec.check(s, k, obs["buffers"][k], w * v, w * b32[k], cap=(1e-4, 1e-5))
    # the slack's reach, from the oracle alone (assert_cap)
    shares = {}
    for name, sl, b in (("dbeta", slack["dbeta"], b_db), ("dthetad", slack["dthetad"], b_dth)):
        shares[name] = 0.0 if sl is None else float((sl > b).double().mean())
    return shares


def assert_cap(shares_by_step):
    """The condition that keeps the slack from hiding a failure: in every step at most half of
    the elements of dbeta and of d theta_d carry a slack above their fp32-rule bound."""
    over = [f"step {s}: {v:.3f} of {k}'s elements carry a slack above their fp32-rule bound"
            for s, sh in enumerate(shares_by_step) for k, v in sh.items() if not v <= SLACK_CAP]
    assert not over, "\n".join(over) + f"\n(cap {SLACK_CAP}: change the corpus, not the cap)"


# ---------------------------------------------------------------- the walk on an engine
def _rows(t, n_tiles, B, ld, nb, V):
    """[n_tiles][B][ld] tiles -> the live rows [nb, V]."""
    return t[: n_tiles * B * ld].view(n_tiles, B, ld)[:, :nb, :64].permute(1, 0, 2).reshape(nb, -1)[:, :V].clone()


def observe(e, model, data, plan_b, s, nb):
    """What step ``s`` left in the engine's workspace, as check_bf16_step reads it."""
    m = e._m
    K, V, B = int(m.K), int(m.V), int(e.bmax)
    obs = {"thetad": e.ws["thetad"][:nb, :K].clone(),
           "kl": e.ws["kl"][:nb].clone(), "rl": e.ws["rl"][:nb].clone(), "loss": e.loss_hist[s].clone(),
           "grads": {k: e.gradient(k).detach().clone() for k, _ in e.param_order},
           "buffers": _buffers(model)}
    n_slab = int(m.n_dpart)
    slabs = e.ws["dthetad"][: n_slab * B * K].view(n_slab, B, K)[:, :nb].double()
    obs["dthetad"] = slabs.sum(0)
    obs["dthetad_slabs"] = (n_slab, slabs.abs().sum(0))
    obs["dtheta"] = e.ws["dtheta"][:nb, :K].clone()
    if m.ctx_fused == 1:
        obs["actx"] = _rows(e.ws["actx"], int(m.n_tiles), B, 64, nb, V)
    from gfedntm_amd.ops import kernel_abi as abi
    if m.kind == abi.KIND_PRODLDA:
        if m.bwd_pre == 2:                       # prodlda_dlogit's tiles, verbatim [B][66]
            obs["dlogit"] = _rows(e.ws["dt"], int(m.n_tiles), B, 66, nb, V)
    else:
        g = torch.zeros(nb, V, device=e.ws["rl"].device)
        ip = data.indptr.cpu().numpy()
        for b, d in enumerate(plan_b):
            e0, e1 = int(ip[d]), int(ip[d + 1])
            g[b, data.indices[e0:e1].long()] = e.ws["dbsm"][e0:e1]
        obs["g"] = g
    return obs


def walk_bf16(fused_tm, data, plan, n_steps, rounding, case="", fed_scale=None):
    """oracle_walk.walk for a matmul_dtype = "bf16" engine in gradient mode: steps
    0 .. n_steps - 1 of ``plan``, each checked by check_bf16_step under ``rounding`` (a Plan)
    from the engine's own state before the step; the batch the device prepared, the counters,
    the noise and Adam in isolation exactly as walk does.  Prints the PARITY lines and the
    ambiguous shares; raises on a tensor over its bound, then on a step over the slack's cap;
    returns (Parity, worst shares)."""
    from gfedntm_amd.ops import kernel_abi as abi
    from gfedntm_amd.ops.engine import UPDATE_GRAD
    e = fused_tm.engine
    assert e.update_mode == UPDATE_GRAD and e._m.mm_bf16 == 1
    assert e.fedavg_scale == fed_scale
    w = 1.0 if fed_scale is None else float(fed_scale)
    rec = Parity(case)
    m64 = copy.deepcopy(fused_tm.model).double()
    m32 = copy.deepcopy(fused_tm.model)
    opt = make_optimizer(list(m64.parameters()), "adam", e.lr, e.beta1)
    assert opt.param_groups[0]["betas"] == (e.beta1, e.beta2)
    kl_w = float(fused_tm.weights.get("beta", 1.0))
    keep = 1.0 / (1.0 - float(fused_tm.dropout))
    prev = None
    worst = {"dbeta": 0.0, "dthetad": 0.0}
    per_step = []
    try:
        for s in range(n_steps):
            sd = {k: v.detach().clone() for k, v in fused_tm.model.state_dict().items()}
            m64.load_state_dict(sd)
            m32.load_state_dict(sd)
            if fed_scale is None:
                e.compute_grads(s)
            else:
                e.sync_step_counter(s)
                e.run_phases([p for p in e.phases() if p != abi.PH_ADAM])
                e.advance_host_step(s)
            torch.cuda.synchronize()
            nb = int(e.ws["nb"].item())
            assert nb == int(plan.size[s]), (s, nb, int(plan.size[s]))
            assert np.array_equal(e.ws["doc"][:nb].cpu().numpy(), plan.batch(s)), s
            assert int(e.d_step.item()) == s + 1, (s, int(e.d_step.item()))
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
            ids = torch.from_numpy(plan.batch(s).astype(np.int64)).to(data.device)
            x = data.dense_rows(ids)
            xc = data.contextual[ids] if data.contextual is not None else None
            obs = observe(e, fused_tm.model, data, plan.batch(s), s, nb)
            shares = check_bf16_step(rec, s, m64, m32, obs, x, xc, (eps, mask_h, mask_t), rounding, kl_w, w)
            per_step.append(shares)
            for k in worst:
                worst[k] = max(worst[k], shares[k])
            for k, v in obs["buffers"].items():
                if "num_batches" in k:
                    assert int(v) == s + 1, (s, k, int(v))
            # the optimizer in isolation: torch Adam in float64 on the kernel's own gradients
            for k, p in m64.named_parameters():
                p.grad = obs["grads"][k].double()
            opt.step()
            e.apply_grads(s)
            torch.cuda.synchronize()
            sd_f = fused_tm.model.state_dict()
            for k, p in m64.named_parameters():
                torch.testing.assert_close(sd_f[k].double(), w * p.detach(), rtol=1e-4, atol=1e-5,
                                           msg=lambda m, k=k: f"step {s} {k} after Adam: {m}")
            assert int(e.adam_t.item()) == s + 1
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
        print(f"PARITY {case} | ambiguous share | dbeta {worst['dbeta']:.3f} | dthetad {worst['dthetad']:.3f} "
              "| per step "
              + " ".join(f"{sh['dbeta']:.3f}/{sh['dthetad']:.3f}" for sh in per_step))
    assert not rec.failures, "\n".join(rec.failures)
    assert_cap(per_step)
    return rec, worst
