"""matmul_dtype = "bf16" against the split float64 oracle of tests/bf16_walk.py: one epoch plus
two steps on tests/helpers.edge_csr (partial last batch, empty documents, dead rows, the epoch
wrap), one case per bf16 kernel instance the launchers can pick (csrc/prodlda.hip kFwdTile /
kFwdStrip / kBwd ``BF`` rows, csrc/ctx.hip gfk_ctx_fwd_rs_k<BF>, the mm_bf16 branches of
csrc/neurallda.hip).  Every case asserts the instance or plan it is about before it walks, and
derives the oracle's rounding plan from the engine (FusedEngine.gemm_dtypes).
"""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan, DeviceCSR
from gfedntm_amd.models import AVITM, CombinedTM
from gfedntm_amd.ops import kernel_abi as abi
from gfedntm_amd.ops.engine import (STAGE_CTX_FULL, STAGE_CTX_RS, STAGE_FWD_POSTFOLD, STAGE_FWD_STRIP,
                                    STAGE_LB, UPDATE_FUSED, UPDATE_GRAD)
from tests.bf16_walk import Plan, walk_bf16
from tests.helpers import edge_csr
from tests.oracle_walk import NOISE_KEYS, check_edges, walk

pytestmark = pytest.mark.gpu

H2 = (32, 24)
FED_W = 0.75
ALL = Plan(True, True, True)


def _build(kind, B, V, K, H, C=20, mode=UPDATE_GRAD):
    torch.manual_seed(0)
    kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=B, verbose=False,
              device="cuda", backend="fused", matmul_dtype="bf16")
    if kind == "combined":
        tm = CombinedTM(contextual_size=C, model_type="prodLDA", **kw)
    else:
        tm = AVITM(model_type=kind, **kw)
    assert tm.backend == "fused" and tm.engine._m.mm_bf16 == 1
    if mode == UPDATE_GRAD:
        tm.engine.set_update_mode(UPDATE_GRAD)
    return tm


def _corpus(kind, B, n_docs, V, nb, C=20, nnz=40):
    per_epoch = -(-n_docs // B)
    n_steps = per_epoch + 2                      # one epoch, then across the wrap
    plan = BatchPlan.build(n_docs, B, n_steps, seed=0)
    s_partial = per_epoch - 1
    assert int(plan.size[s_partial]) == nb and int(plan.epoch[n_steps - 1]) == 1
    X, marks = edge_csr(n_docs, V, nnz, plan, s_partial, seed=1)
    check_edges(X, marks, plan, s_partial, n_steps)
    ctx = None
    if kind == "combined":
        ctx = np.random.default_rng(2).standard_normal((n_docs, C)).astype(np.float32)
    return DeviceCSR(X, "cuda", contextual=ctx), plan, n_steps


def _twin(tm, kind, B, V, K, H, data, plan):
    """The production path on the walked plan: fused optimizer epilogues, graph replay, the
    FedAvg pre-scale (as tests/test_epoch_walk_gpu.py)."""
    b = _build(kind, B, V, K, H, mode=UPDATE_FUSED)
    e = b.engine
    assert e.update_mode == UPDATE_FUSED and e._m.stage_flags == tm.engine._m.stage_flags
    assert e.gemm_dtypes == tm.engine.gemm_dtypes
    b.model.load_state_dict(tm.model.state_dict())
    e.seed = e._m.seed = tm.engine.seed
    e.set_fedavg_scale(FED_W)
    e.bind_data(data, plan)
    e.enable_graph(True)
    return b


def _compare_twin(a, b, n_steps):
    e, half = b.engine, n_steps // 2
    for s in range(half):
        e.step(s)
    e.step_k(half, n_steps - half)
    torch.cuda.synchronize()
    torch.testing.assert_close(e.loss_hist, a.engine.loss_hist, rtol=1e-4, atol=1e-2)
    assert int(e.d_step.item()) == int(e.adam_t.item()) == n_steps
    sa, sb = b.model.state_dict(), a.model.state_dict()
    lr_steps = 2 * a.engine.lr * n_steps
    for k in sb:
        if not sb[k].is_floating_point():
            assert torch.equal(sa[k], sb[k]), k
            continue
        noisy = k in NOISE_KEYS or k.startswith(("inf_net.f_mu_batchnorm.running_mean",
                                                 "inf_net.f_sigma_batchnorm.running_mean"))
        torch.testing.assert_close(sa[k], sb[k], rtol=1e-3, atol=lr_steps if noisy else 5e-5,
                                   msg=lambda m, k=k: f"twin {k}: {m}")


def _walk_case(case, kind, B, n_docs, nb, K, H, V=701, C=20, expect=None, rounding=ALL, twin=False,
               nnz=40):
    """Build, assert the instance the case is about (``expect(engine)``) and that the engine's
    own account of its GEMMs is the plan the case names, walk."""
    tm = _build(kind, B, V, K, H, C=C)
    e = tm.engine
    if expect is not None:
        expect(e)
    assert Plan.of(e.gemm_dtypes) == rounding, (e.gemm_dtypes, rounding)
    data, plan, n_steps = _corpus(kind, B, n_docs, V, nb, C=C, nnz=nnz)
    b = None
    if twin:
        e.set_fedavg_scale(FED_W)
        b = _twin(tm, kind, B, V, K, H, data, plan)
    e.bind_data(data, plan)
    out = walk_bf16(tm, data, plan, n_steps, rounding, case=case, fed_scale=FED_W if twin else None)
    if twin:
        _compare_twin(tm, b, n_steps)
    return out


def _flags(e):
    return int(e._m.stage_flags)


def _tile_bwd(e, bm):
    """The tile backward (one workgroup per tile, one k range), no stored logit gradient."""
    m = e._m
    assert e.bmax == bm and m.n_dpart == m.n_tiles and m.bwd_pre == 0 and not e.large_batch


def test_a_strip_bm16_np8_tile_backward_bm16():
    """ProdLDA B = 16, K = 20: prodlda_fwd_strip_kernel<16, 8, 3, ., BF> (strip_np_bf(20) = 8
    pairs: one 32-k step) and prodlda_bwd_kernel<16, 1, 1, BF>, whose dbeta takes the 16x16x16
    path (BM % 32 != 0).  37 documents: nb = 5.  With the production twin."""
    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP and not _flags(e) & (2 | STAGE_FWD_POSTFOLD)
        _tile_bwd(e, 16)
    _walk_case("A", "prodLDA", 16, 37, 5, 20, H2, expect=expect, twin=True)


def test_b_strip_bm32_np16_dead_rows_every_batch():
    """B = 24 on the 32-row kernels, K = 72 (16 pairs): every batch has dead rows; nb = 3."""
    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP
        _tile_bwd(e, 32)
    _walk_case("B", "prodLDA", 24, 51, 3, 72, H2, expect=expect)


def test_c_strip_np32_batch_matrices_from_l2():
    """B = 64, K = 200: 32 pairs, stage_flags bit 1, the backward's MAXU = 4; nb = 2."""
    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP and _flags(e) & 2
        _tile_bwd(e, 64)
    _walk_case("C", "prodLDA", 64, 66, 2, 200, (50,), expect=expect)


def test_d_strip_with_postfold(monkeypatch):
    monkeypatch.setenv("GFEDNTM_POSTFOLD", "1")

    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP and _flags(e) & STAGE_FWD_POSTFOLD
        assert abi.PH_POST_FWD not in e.phases()
        _tile_bwd(e, 16)
    _walk_case("D", "prodLDA", 16, 35, 3, 20, H2, expect=expect)


@pytest.mark.parametrize("K", [40, 20])
def test_e_tile_forward(monkeypatch, K):
    """GFEDNTM_FWD_STRIP=0: prodlda_fwd_kernel<32, BF>.  K = 40: round_up(K, 16) = 48, one
    32-k step plus the 16x16x16 tail; K = 20: one 32-k step with 12 padded topics."""
    monkeypatch.setenv("GFEDNTM_FWD_STRIP", "0")

    def expect(e):
        assert e.bmax == 32 and not _flags(e) & STAGE_FWD_STRIP
        _tile_bwd(e, 32)
    _walk_case(f"E{K}", "prodLDA", 24, 51, 3, K, H2, expect=expect)


def test_f_tile_forward_and_backward_bm128():
    """bmax = 128: no strip instance exists, so prodlda_fwd_kernel<128, BF>, and
    prodlda_bwd_kernel<128, 1, 1, BF>.  133 documents: nb = 5."""
    def expect(e):
        assert not _flags(e) & STAGE_FWD_STRIP
        _tile_bwd(e, 128)
    _walk_case("F", "prodLDA", 128, 133, 5, 50, (50, 50), V=2001, expect=expect)


@pytest.mark.parametrize("pre", ["0", "3"])
def test_g_forced_k_split_backward(monkeypatch, pre):
    """K = 256, B = 64, V = 5000 (79 tiles, unpadded rows): the 4-k-range backward.
    GFEDNTM_BWD_PRE=0: prodlda_bwd_kernel<64, 4, 4, BF> recomputing the logit gradient;
    =3: prodlda_bwd_pre2_kernel<64, 4, BF> reading prodlda_dlogit's tiles -- dlogit is checked
    under the rule and forced."""
    monkeypatch.setenv("GFEDNTM_BWD_PRE", pre)

    def expect(e):
        m = e._m
        assert m.n_dpart < m.n_tiles and m.bwd_pre == (2 if pre == "3" else 0) and e.bmax == 64
        assert _flags(e) & STAGE_FWD_STRIP
    _walk_case("G" + ("2" if pre == "3" else "0"), "prodLDA", 64, 67, 3, 256, (50,), V=5000, expect=expect)


def test_g3_pipelined_backward_keeps_fp32_operands():
    """V = 4992 (ldb % 64 == 0): bwd_pre == 3, the pipelined backward, which has no bf16
    instance -- the forward rounds, the backward GEMMs do not, and gemm_dtypes must say so."""
    def expect(e):
        assert e._m.bwd_pre == 3 and e._m.ldb % 64 == 0 and _flags(e) & STAGE_FWD_STRIP
        assert e.gemm_dtypes == {"dec_fwd": "bf16", "dthetad": "fp32", "dbeta": "fp32",
                                 "ctx_a": None, "ctx_z0": None}
    _walk_case("G3", "prodLDA", 64, 67, 3, 256, (50,), V=4992, expect=expect,
               rounding=Plan(True, False, False))


def test_h_neurallda_empty_rows():
    def expect(e):
        assert e._m.kind == abi.KIND_LDA and abi.PH_LDA_BETA_BWD in e.phases() and e.bmax == 16
    _walk_case("H", "LDA", 16, 37, 5, 20, H2, expect=expect, twin=True)


@pytest.mark.parametrize("B,n_docs,nb", [(128, 133, 5), (256, 259, 3)])
def test_i_neurallda_128_row_chunks(B, n_docs, nb):
    """B = 128: one whole 128-row x^T tile (gfk_lda_beta_bwd_k<., ., false>: the chunked ``CH``
    instance is launched for bmax > 128 only, csrc/neurallda.hip gfk_launch_lda_beta_bwd).
    B = 256 is the smallest batch that runs it: the large-batch plan, two chunks, where
    NeuralLDA's kernels still read mm_bf16 (only ProdLDA's large-batch decoder ignores it).
    12 non-zeros per random row instead of 40: d theta_d[b, k] sums bf(beta_sm[k, v]) over row
    b's words, beta_sm is never stored, and at K = 50 with 40 words more than half of its
    elements meet an ambiguous one (0.58 measured; the edge rows keep their 32 words and the
    count of 1000)."""
    def expect(e):
        assert e._m.kind == abi.KIND_LDA and e.bmax == B and e.large_batch == (B > 128)
    _walk_case(f"I{B}", "LDA", B, n_docs, nb, 50, (50, 50), V=2001, expect=expect, nnz=12)


@pytest.mark.parametrize("C", [20, 100, 260])
def test_j_combined_register_streamed_forward(C):
    """gfk_ctx_fwd_rs_k<., BF>: C = 20 is less than one 32-k step, 100 no multiple of 32, 260 a
    second 256-float phase that is 4 wide."""
    def expect(e):
        rs = STAGE_CTX_FULL | STAGE_CTX_RS
        assert e._m.ctx_fused == 1 and (_flags(e) & rs) == rs and e.ctx_gemm_dtype == "bf16"
        assert abi.PH_CTXF_FWD in e.phases() and abi.PH_CTXF_BWD in e.phases()
    _walk_case(f"J{C}", "combined", 16, 35, 3, 20, H2, C=C, expect=expect,
               rounding=Plan(True, True, True, True, True))


def test_l_large_batch_plan_ignores_bf16():
    """B = 256, ProdLDA: the large-batch decoder has no bf16 instance; gemm_dtypes says fp32
    everywhere and the fp32 walk of tests/oracle_walk.py passes unchanged."""
    tm = _build("prodLDA", 256, 3001, 50, (50, 50))
    e = tm.engine
    assert e.large_batch and e.bmax == 256 and _flags(e) & STAGE_LB and (e._m.lb_fused & 3) == 3
    assert e.gemm_dtypes == {"dec_fwd": "fp32", "dthetad": "fp32", "dbeta": "fp32",
                             "ctx_a": None, "ctx_z0": None}
    data, plan, n_steps = _corpus("prodLDA", 256, 259, 3001, 3)
    e.bind_data(data, plan)
    walk(tm, data, plan, n_steps, case="L")
