"""A whole epoch of the fused step against the float64 oracle (tests/oracle_walk.py).

tests/test_fused_kernels.py's _oracle_step checks step 0, a full batch, documents with at
least one word.  These walks run one epoch plus two steps -- so every later step's batch is
the one the update kernels' extra workgroup prepared, the last batch of the epoch is short
(rows >= nb repeat its first document and must stay out of every statistic, product and
1 / nb), the epoch wraps -- on a corpus with empty documents and the other rows of
tests/helpers.edge_csr, on the smallest shapes that reach each kernel family.  Each step is
compared with the oracle from the engine's own state, under the bound of docs/PARITY.md.

The production-mode twins tie the fused optimizer epilogues and graph replay on the same
partial batches to the walked gradient-mode engine (tolerances of
test_fused_update_matches_gradient_mode).
"""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan, DeviceCSR
from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
from gfedntm_amd.ops.engine import (STAGE_CTX_BWDPP, STAGE_CTX_FULL, STAGE_FWD_POSTFOLD,
                                    STAGE_FWD_STRIP, STAGE_LB, STAGE_WIN_SPARSE, UPDATE_FUSED,
                                    UPDATE_GRAD)
from gfedntm_amd.ops import kernel_abi as abi
from tests.helpers import edge_csr
from tests.oracle_walk import NOISE_KEYS, check_edges, walk

pytestmark = pytest.mark.gpu

H2 = (32, 24)
FED_W = 0.75


def _build(kind, B, V, K, H, C=20, mode=UPDATE_GRAD):
    torch.manual_seed(0)
    kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=B, verbose=False,
              device="cuda", backend="fused")
    if kind in ("combined", "zeroshot"):
        cls = CombinedTM if kind == "combined" else ZeroShotTM
        tm = cls(contextual_size=C, model_type="prodLDA", **kw)
    else:
        tm = AVITM(model_type=kind, **kw)
    assert tm.backend == "fused"
    if mode == UPDATE_GRAD:
        tm.engine.set_update_mode(UPDATE_GRAD)
    return tm


def _corpus(kind, B, n_docs, V, nb, C=20):
    per_epoch = -(-n_docs // B)
    n_steps = per_epoch + 2                      # one epoch, then across the wrap
    plan = BatchPlan.build(n_docs, B, n_steps, seed=0)
    s_partial = per_epoch - 1
    assert int(plan.size[s_partial]) == nb and int(plan.epoch[n_steps - 1]) == 1
    X, marks = edge_csr(n_docs, V, 40, plan, s_partial, seed=1)
    check_edges(X, marks, plan, s_partial, n_steps)
    ctx = None
    if kind in ("combined", "zeroshot"):
        ctx = np.random.default_rng(2).standard_normal((n_docs, C)).astype(np.float32)
    return DeviceCSR(X, "cuda", contextual=ctx), plan, n_steps


def _twin(tm, kind, B, V, K, H, data, plan, n_steps):
    """The production path on the walked plan: fused optimizer epilogues, graph replay, the
    FedAvg pre-scale; the first half of the steps by step(), the rest in one step_k()."""
    b = _build(kind, B, V, K, H, mode=UPDATE_FUSED)
    e = b.engine
    assert e.update_mode == UPDATE_FUSED and e._m.stage_flags == tm.engine._m.stage_flags
    b.model.load_state_dict(tm.model.state_dict())
    e.seed = e._m.seed = tm.engine.seed
    e.set_fedavg_scale(FED_W)
    e.bind_data(data, plan)
    e.enable_graph(True)
    return b


def _run_twin(b, n_steps):
    e, half = b.engine, n_steps // 2
    for s in range(half):
        e.step(s)
    e.step_k(half, n_steps - half)
    torch.cuda.synchronize()


def _compare_twin(a, b, n_steps):
    torch.testing.assert_close(b.engine.loss_hist, a.engine.loss_hist, rtol=1e-4, atol=1e-2)
    assert int(b.engine.d_step.item()) == int(b.engine.adam_t.item()) == n_steps
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


def _walk_case(case, kind, B, n_docs, nb, K, H, V=701, expect=None, twin=False):
    """Build, assert the plan the case is about (``expect(engine)``), walk; with ``twin``
    both engines carry the FedAvg pre-scale and the twin must land on the walked state."""
    tm = _build(kind, B, V, K, H)
    e = tm.engine
    if expect is not None:
        expect(e)
    data, plan, n_steps = _corpus(kind, B, n_docs, V, nb)
    b = None
    if twin:
        e.set_fedavg_scale(FED_W)
        b = _twin(tm, kind, B, V, K, H, data, plan, n_steps)
    e.bind_data(data, plan)
    rec = walk(tm, data, plan, n_steps, case=case, fed_scale=FED_W if twin else None)
    if twin:
        _run_twin(b, n_steps)
        _compare_twin(tm, b, n_steps)
    return rec


def _flags(e):
    return int(e._m.stage_flags)


def test_a_strip_forward_staged_plan():
    """ProdLDA, B = 16, 37 documents: nb = 5; the strip forward, batch matrices in LDS."""
    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP and not _flags(e) & 2 and not e.large_batch
        assert not _flags(e) & (STAGE_FWD_POSTFOLD | STAGE_WIN_SPARSE)
    _walk_case("a", "prodLDA", 16, 37, 5, 20, H2, expect=expect, twin=True)


def test_b_tile_forward_every_batch_has_dead_rows(monkeypatch):
    """batch_size 24 on the 32-row kernels (GFEDNTM_FWD_STRIP=0: the tile forward): every
    batch of the epoch has dead rows, the last one 29 of them."""
    monkeypatch.setenv("GFEDNTM_FWD_STRIP", "0")

    def expect(e):
        assert e.bmax == 32 and not _flags(e) & STAGE_FWD_STRIP
    _walk_case("b", "prodLDA", 24, 51, 3, 20, H2, expect=expect)


def test_c_posterior_folded_into_forward(monkeypatch):
    monkeypatch.setenv("GFEDNTM_POSTFOLD", "1")

    def expect(e):
        assert _flags(e) & STAGE_FWD_POSTFOLD and abi.PH_POST_FWD not in e.phases()
    _walk_case("c", "prodLDA", 16, 35, 3, 20, H2, expect=expect)


def test_d_batch_matrices_from_l2():
    """K = 200, B = 64: stage_flags bit 1; 66 documents: nb = 2, the smallest batch with a
    variance."""
    def expect(e):
        assert _flags(e) & 2 and not e.large_batch
    _walk_case("d", "prodLDA", 64, 66, 2, 200, (50,), expect=expect, twin=True)


@pytest.mark.parametrize("pre", ["3", "0"])
def test_e_forced_k_split_backward(monkeypatch, pre):
    """K = 256, B = 64, 79 tiles: the 4-k-range persistent backward forced by the LDS
    (n_dpart < n_tiles), its logit-gradient tiles from prodlda_dlogit (GFEDNTM_BWD_PRE=3; the
    unpadded V = 5000 rows run its two-per-CU kernel) or recomputed per range (=0)."""
    monkeypatch.setenv("GFEDNTM_BWD_PRE", pre)

    def expect(e):
        m = e._m
        assert m.n_dpart < m.n_tiles and m.bwd_pre == (2 if pre == "3" else 0)
    _walk_case("e" + pre, "prodLDA", 64, 67, 3, 256, (50,), V=5000, expect=expect)


def test_f_sparse_win_tiles_one_dead_row(monkeypatch):
    monkeypatch.setenv("GFEDNTM_WIN_SPARSE", "1")

    def expect(e):
        assert _flags(e) & STAGE_WIN_SPARSE
    _walk_case("f", "prodLDA", 32, 63, 31, 20, H2, expect=expect, twin=True)


def test_g_one_row_batch():
    """33 documents, B = 16: the epoch's last batch is one row (an empty document here).
    Batch norm of one row: variance 0, the running variance fed that 0 (the engine's
    convention, oracle_walk._bn_train), no gradient through the normalised heads."""
    _walk_case("g", "prodLDA", 16, 33, 1, 20, H2)


def test_h_neurallda_empty_rows():
    def expect(e):
        assert e._m.kind == abi.KIND_LDA and abi.PH_LDA_BETA_BWD in e.phases()
    _walk_case("h", "LDA", 16, 37, 5, 20, H2, expect=expect, twin=True)


def test_i_neurallda_128_row_chunks():
    def expect(e):
        assert e._m.kind == abi.KIND_LDA and e.bmax == 128 and not e.large_batch
    _walk_case("i", "LDA", 128, 133, 5, 50, (50, 50), V=2001, expect=expect)


@pytest.mark.parametrize("forced", [False, True])
def test_j_combined_ctx_kernels(monkeypatch, forced):
    """CombinedTM, C = 20: ctx_fwd / ctx_bwd on their default small-V shapes, then the
    large-V ones forced (all rows per tile; the persistent pipelined backward)."""
    if forced:
        monkeypatch.setenv("GFEDNTM_CTX_FULL", "1")
        monkeypatch.setenv("GFEDNTM_CTX_BWDPP", "1")

    def expect(e):
        assert e._m.ctx_fused == 1 and abi.PH_CTXF_FWD in e.phases() and abi.PH_CTXF_BWD in e.phases()
        assert bool(_flags(e) & STAGE_CTX_FULL) == forced
        assert bool(_flags(e) & STAGE_CTX_BWDPP) == forced
    _walk_case("j" + ("-full" if forced else ""), "combined", 16, 35, 3, 20, H2, expect=expect,
               twin=True)


def test_k_zeroshot_dense_input_layer():
    def expect(e):
        assert e._m.ctx_fused == 2
    _walk_case("k", "zeroshot", 16, 35, 3, 20, H2, expect=expect)


@pytest.mark.parametrize("kind", ["prodLDA", "LDA"])
def test_l_large_batch_253_dead_rows(kind):
    """B = 256, 259 documents: the large-batch plan (ProdLDA: the MFMA decoder kernels) on a
    last batch of 3 live rows and 253 dead ones."""
    def expect(e):
        assert e.large_batch and e.bmax == 256 and _flags(e) & STAGE_LB
        if kind == "prodLDA":
            assert e._m.lb_fused == 3 and abi.PH_LB_GEMM_FWD not in e.phases()
    _walk_case("l-" + kind, kind, 256, 259, 3, 50, (50, 50), V=3001, expect=expect)
