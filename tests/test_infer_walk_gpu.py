"""Every instance of the theta-inference kernel (csrc/infer.hip: Staged x NQ {1, 2, 4, 8} x
KQ {1, 2, 3, 4, 8}) against the float64 oracle of tests/infer_oracle.py, on the corpus of
tests/helpers.row_edge_csr -- empty documents, rows of 63 / 64 / 65 / 127 / 128 / 129 / 400
non-zeros, a count of 1000 -- under the bound of docs/PARITY.md section 4.1:

    e_kernel <= 8 e_fp32 + 4 * 2^-23 * scale

with e_fp32 the error of the fp32 eval-mode torch encoder on the same state and documents,
evaluated for the count-1000 document and for the other rows apart, and elementwise never
looser than rtol 1e-4 / atol 1e-4.  No model is trained: ``perturb_state`` loads running
statistics and weights no initialisation gives, so that the pre-activations reach past 20
(the softplus identity branch) and below -5 (the negative arms), asserted on the oracle.

Each case asserts the kernel variant it reaches.  Two of the 2 x 4 x 5 instances cannot be
reached through the engine: NQ = 8 with KQ = 8 (K > 256 runs the large-batch plan, which
takes hidden_sizes[0] <= 64), staged or not; case G is therefore split into the unstaged
NQ = 8 / KQ = 4 and the unstaged NQ = 1 / KQ = 8.

The theta means are compared with ``oracle_theta`` fed the kernel's own moments and the numpy
Philox draws, at rtol 1e-4 / atol 2e-5, and measured against an fp32 numpy restatement of the
same formula (its Box-Muller in fp32 from the same Philox integers), under the same rule
(docs/PARITY.md section 4.2 has the ratios).
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import DeviceCSR
from gfedntm_amd.eval.export import postprocess_thetas
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from gfedntm_amd.models.networks import ACTIVATIONS
from gfedntm_amd.ops import kernel_abi as abi
from tests.helpers import row_edge_csr
from tests.infer_oracle import (edge_context, infer_normals, oracle_moments, oracle_theta, parity,
                                perturb_state)

pytestmark = pytest.mark.gpu

V, CTX, LAB = 701, 20, 5
SEED = 0x1234_5678_9ABC
STAGED_LIMIT = 160 * 1024
CAP = (1e-4, 1e-4)                       # today's elementwise tolerance of the moments
X, MARKS = row_edge_csr(V, seed=1)
N = X.shape[0]
HOT = np.array([MARKS["count1000"]])
REST = np.setdiff1d(np.arange(N), HOT)
EMB, LABELS = edge_context(N, CTX, LAB, MARKS)

# name: (kind, hidden sizes, K, (staged, NQ, KQ))
CASES = {
    "A": ("prodLDA", (32, 24), 20, (True, 1, 1)),
    "B": ("prodLDA", (100,), 100, (True, 2, 2)),
    "C": ("prodLDA", (200, 64), 130, (True, 4, 3)),
    "D": ("prodLDA", (512, 16), 200, (True, 8, 4)),
    "E": ("prodLDA", (32, 24), 300, (True, 1, 8)),
    "F": ("prodLDA", (200, 200), 50, (False, 4, 1)),
    "G-nq8": ("prodLDA", (320,), 256, (False, 8, 4)),
    "G-kq8": ("prodLDA", (64,), 300, (False, 1, 8)),
    "H-staged": ("prodLDA", (170, 170), 20, (True, 4, 1)),
    "H-unstaged": ("prodLDA", (176, 176), 20, (False, 4, 1)),
    "I": ("prodLDA", (16,) * abi.MAX_LAYERS, 20, (True, 1, 1)),
    "J": ("LDA", (32, 24), 20, (True, 1, 1)),
    "K-combined": ("combined", (32, 24), 20, (True, 1, 1)),
    "K-zeroshot": ("zeroshot", (32, 24), 20, (True, 1, 1)),
    "K-labels": ("combined+labels", (32, 24), 20, (True, 1, 1)),
}

_MODELS = {}


def _model(case, activation="softplus"):
    """(tm, data, ctx, labels) of a case, built once per module: the fused engine, a
    perturbed state, the edge corpus on the device."""
    key = (case, activation)
    if key not in _MODELS:
        kind, H, K, _ = CASES[case]
        torch.manual_seed(0)
        kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=16, verbose=False,
                  device="cuda", backend="fused", activation=activation)
        ctx = labels = None
        if kind in ("prodLDA", "LDA"):
            tm = AVITM(model_type=kind, **kw)
        else:
            cls = ZeroShotTM if kind == "zeroshot" else CombinedTM
            ctx, labels = EMB, (LABELS if kind.endswith("labels") else None)
            tm = cls(contextual_size=CTX, model_type="prodLDA", label_size=LAB if labels is not None else 0,
                     **kw)
        assert tm.backend == "fused"
        perturb_state(tm, seed=3)
        torch.cuda.synchronize()
        _MODELS[key] = (tm, DeviceCSR(X, "cuda", contextual=ctx, labels=labels), ctx, labels)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _instance(tm):
    """(staged, NQ, KQ) of the gfk_theta_infer_k instance the launcher picks (csrc/infer.hip
    launch_nq / launch_kq), and the staged variant's LDS bytes."""
    m = tm.engine._m
    smem = int(tm.engine.lib.gfk_theta_infer_smem(C.byref(m)))
    h0, kq = int(m.H[0]), -(-int(m.K) // 64)
    nq = next(q for q in (1, 2, 4, 8) if h0 <= 64 * q)
    return (smem <= STAGED_LIMIT, nq, kq if kq <= 4 else 8), smem


def _fp32_moments(tm, data):
    tm.model.eval()
    x = torch.from_numpy(X.toarray()).cuda()
    with torch.no_grad():
        if tm.kind == "ctm":
            return tm.model.inf_net(x, data.contextual, data.labels)
        return tm.model.inf_net(x)


def _check_moments(case, activation="softplus"):
    tm, data, ctx, labels = _model(case, activation)
    inst, smem = _instance(tm)
    print(f"INFER {case} {activation} | instance staged={inst[0]} NQ={inst[1]} KQ={inst[2]} | "
          f"staged LDS {smem} B")
    assert inst == CASES[case][3], (inst, smem)
    assert len(tm.hidden_sizes) == int(tm.engine._m.n_hidden)
    mu64, ls64, pre = oracle_moments(tm, X, ctx, labels, return_pre=True)
    assert np.isfinite(mu64).all() and np.isfinite(ls64).all()
    assert pre[0].max() > 20.0 and pre[0].min() < -5.0            # both softplus branches, the negative arms
    mom = tm.engine.theta_infer(data, moments=True).double().cpu().numpy()
    mu32, ls32 = (t.double().cpu().numpy() for t in _fp32_moments(tm, data))
    failures = []
    for name, got, f64, f32 in (("mu", mom[:, 0], mu64, mu32), ("ls", mom[:, 1], ls64, ls32)):
        for rows_name, rows in (("count1000", HOT), ("rest", REST)):
            p = parity(got, f64, f32, rows=rows, cap=CAP)
            print(f"INFER-PARITY {case} {activation} | {name} | {rows_name} | e_kernel {p['e_kernel']:.3e} | "
                  f"e_fp32 {p['e_fp32']:.3e} | scale {p['scale']:.3e} | e_kernel/e_fp32 {p['ratio']:.2f} | "
                  f"bound used {p['use']:.3f}")
            if not p["ok"]:
                failures.append((name, rows_name, p))
    assert not failures, failures
    return mom


@pytest.mark.parametrize("activation", ACTIVATIONS)
def test_a_every_activation(activation):
    """Staged, NQ 1, KQ 1: all eight arms of act_f in eval mode."""
    _check_moments("A", activation)


@pytest.mark.parametrize("case", [c for c in CASES if c != "A"])
def test_moments(case):
    _check_moments(case)


def test_h_pair_straddles_the_staging_limit():
    """(170, 170) is the largest staged request of the suite, (176, 176) the first unstaged."""
    (sa, _, _), a = _instance(_model("H-staged")[0])
    (sb, _, _), b = _instance(_model("H-unstaged")[0])
    assert sa and not sb and 150 * 1024 < a <= STAGED_LIMIT < b < 165 * 1024


# ------------------------------------------------------------------ theta means
THETA_TOL = dict(rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("S", [1, 4, 5, 20])
@pytest.mark.parametrize("case", ["A", "C", "E", "G-nq8", "G-kq8", "K-combined"])
def test_theta_mean(case, S):
    """S = 1, 4, 5, 20: one draw, a whole Philox block, a block and a quarter, the default."""
    tm, data, _, _ = _model(case)
    K = CASES[case][2]
    mom = tm.engine.theta_infer(data, moments=True)
    th = tm.engine.theta_infer(data, n_samples=S, seed=SEED).double().cpu().numpy()
    mom = mom.cpu().numpy()
    mu, ls = mom[:, 0], mom[:, 1]
    print(f"INFER-THETA {case} S={S} | max |mu| {np.abs(mu).max():.3g} | max ls {ls.max():.3g} | "
          f"min ls {ls.min():.3g}")
    ref = oracle_theta(mu, ls, infer_normals(SEED, N, K, S))
    f32 = oracle_theta(mu, ls, infer_normals(SEED, N, K, S, dtype=np.float32), dtype=np.float32)
    assert np.isfinite(th).all()
    failures = []
    for rows_name, rows in (("count1000", HOT), ("rest", REST)):
        p = parity(th, ref, f32, rows=rows)
        if not p["ok"]:
            failures.append((rows_name, p))
        print(f"INFER-PARITY {case} S={S} | theta | {rows_name} | e_kernel {p['e_kernel']:.3e} | "
              f"e_fp32 {p['e_fp32']:.3e} | scale {p['scale']:.3e} | e_kernel/e_fp32 {p['ratio']:.2f} | "
              f"bound used {p['use']:.3f}")
    np.testing.assert_allclose(th, ref, **THETA_TOL)
    np.testing.assert_allclose(th.sum(1), 1.0, atol=1e-5)
    assert not failures, failures           # the 8x rule holds for theta too (PARITY.md 4.2)


# ------------------------------------------------------------------ post-processing
def test_postprocess_thresholds():
    tm, data, _, _ = _model("A")
    e, S = tm.engine, 20
    th = e.theta_infer(data, n_samples=S, seed=5)
    thr = float(np.float32(3e-3))
    pp = e.theta_infer(data, n_samples=S, seed=5, postprocess=True, threshold=thr).cpu().numpy()
    ref = postprocess_thetas(th.cpu().numpy(), thr)
    zeroed = (ref == 0) & (th.cpu().numpy() > 0)
    assert zeroed.any() and not zeroed.all(1).any()               # some entries, no whole row
    np.testing.assert_allclose(pp, ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(pp == 0, ref == 0)
    # a threshold above every entry of a row: tot == 0, the row stays exactly zero
    mom = e.theta_infer(data, moments=True).cpu().numpy()
    plain = oracle_theta(mom[:, 0], mom[:, 1], infer_normals(5, N, 20, S))
    ora = oracle_theta(mom[:, 0], mom[:, 1], infer_normals(5, N, 20, S), threshold=0.9)
    all_zero = plain.max(1) < 0.9 - 1e-3                          # (clear of the threshold in fp32 too)
    one_hot = plain.max(1) > 0.9 + 1e-3
    assert all_zero.sum() >= 1 and (ora[all_zero] == 0).all()
    hi = e.theta_infer(data, n_samples=S, seed=5, postprocess=True, threshold=0.9).cpu().numpy()
    print("POSTPROCESS rows all under 0.9:", int(all_zero.sum()), "rows with one entry over:", int(one_hot.sum()))
    assert np.isfinite(hi).all()
    assert (hi[all_zero] == 0).all()
    # one entry over: it alone survives, x * (1 / x) within an ulp of 1
    assert ((hi[one_hot] != 0).sum(1) == 1).all() and (np.abs(hi[one_hot].max(1) - 1) <= 2.0 ** -22).all()
    # the median of the oracle's row maxima as the threshold: all-zero rows next to rows that keep
    # their top entries, in one launch
    mid = float(np.float32(np.median(plain.max(1))))
    zero_rows, live_rows = plain.max(1) < mid - 1e-3, plain.max(1) > mid + 1e-3
    assert zero_rows.sum() >= 10 and live_rows.sum() >= 10
    got = e.theta_infer(data, n_samples=S, seed=5, postprocess=True, threshold=mid).cpu().numpy()
    ref = postprocess_thetas(th.cpu().numpy(), mid)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6)
    np.testing.assert_array_equal(got == 0, ref == 0)
    assert (got[zero_rows] == 0).all() and np.allclose(got[live_rows].sum(1), 1.0, atol=1e-6)


# ------------------------------------------------------------------ chunking
@pytest.mark.parametrize("case", ["A", "K-combined", "K-zeroshot", "K-labels", "F"])
def test_chunks_are_bitwise_equal(case):
    """chunk = 37 and 64: later launches have doc0 != 0 -- the draw key, the output offset,
    and for CTM the chunk-local rows of a sliced hctx (contextual and label slices)."""
    tm, data, _, _ = _model(case)
    e = tm.engine
    mom = e.theta_infer(data, moments=True)
    th = e.theta_infer(data, n_samples=5, seed=SEED)
    assert not torch.equal(th[:37], th[37:74])
    for chunk in (37, 64):
        assert torch.equal(mom, e.theta_infer(data, moments=True, chunk=chunk)), chunk
        assert torch.equal(th, e.theta_infer(data, n_samples=5, seed=SEED, chunk=chunk)), chunk
