"""The production update mode against the float64 oracle, step by step (tests/fused_walk.py):
Adam and the FedAvg pre-scale in the kernels' epilogues, no gradient materialised.

(a) One client: the shapes and plan assertions of tests/test_epoch_walk_gpu.py whose step has
an Adam epilogue of its own, run eagerly (the twins there keep covering graph replay).

(b) Several clients in ONE BatchedSteps launch (grid z = client), captured and replayed as
MultiClientRound.time_local_steps does.  The clients have their own seeds, corpora and
document counts, so within one launch one client is on a full batch, another on a partial one
(down to one and two rows), and their epochs wrap at different steps; there is no fold and no
shared read copy, so they diverge, and each is compared with the oracle from its own state.
These are the GB = true instances (the 8-wave prodlda_bwd8_kernel, win_update's 8-wave tiles at
6 and 8 waves per SIMD, the joint post_bwd rows, the M-client strip fill, the posterior folded
for M > 1), which have no gradient mode and were tied to the one-client kernels bit for bit only.

Every case runs one epoch of its shortest client plus two steps on tests/helpers.edge_csr
corpora and prints its PARITY lines (docs/PARITY.md section 4.1 carries them).
"""
import numpy as np
import pytest
import torch

from gfedntm_amd.data.bow import BatchPlan, DeviceCSR
from gfedntm_amd.models import AVITM, CombinedTM
from gfedntm_amd.ops import kernel_abi as abi
from gfedntm_amd.ops.engine import (STAGE_BWD_BATCH8, STAGE_CTX_BWDPP, STAGE_CTX_FULL, STAGE_FWD_POSTFOLD,
                                    STAGE_FWD_STRIP, STAGE_LB, STAGE_POST_JOINT, STAGE_POST_ROWS2,
                                    STAGE_POST_ROWS4, STAGE_WIN_BATCH8, STAGE_WIN_SPARSE,
                                    STAGE_WIN_WAVES6, UPDATE_FUSED, BatchedSteps)
from gfedntm_amd.utils.misc import graph_capture
from tests.fused_walk import walk_fused
from tests.helpers import edge_csr
from tests.oracle_walk import check_edges
from tests.test_epoch_walk_gpu import FED_W, H2, _build, _corpus, _flags

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- (a) one client
def _one(case, kind, B, n_docs, nb, K, H, V=701, expect=None, scaled=False):
    tm = _build(kind, B, V, K, H, mode=UPDATE_FUSED)
    e = tm.engine
    assert e.update_mode == UPDATE_FUSED or e.large_batch
    if expect is not None:
        expect(e)
    data, plan, n_steps = _corpus(kind, B, n_docs, V, nb)
    w = FED_W if scaled else None
    e.set_fedavg_scale(w)
    e.bind_data(data, plan)
    return walk_fused([tm], [data], [plan], n_steps, case, fed_scales=[w])


def test_a_strip_forward():
    def expect(e):
        assert _flags(e) & STAGE_FWD_STRIP and not _flags(e) & 2 and not e.large_batch
        assert not _flags(e) & (STAGE_FWD_POSTFOLD | STAGE_WIN_SPARSE)
    _one("fused a", "prodLDA", 16, 37, 5, 20, H2, expect=expect, scaled=True)


def test_d_batch_matrices_from_l2():
    def expect(e):
        assert _flags(e) & 2 and not e.large_batch
    _one("fused d", "prodLDA", 64, 66, 2, 200, (50,), expect=expect)


@pytest.mark.parametrize("pre", ["3", "0"])
def test_e_forced_k_split_backward(monkeypatch, pre):
    monkeypatch.setenv("GFEDNTM_BWD_PRE", pre)

    def expect(e):
        m = e._m
        assert m.n_dpart < m.n_tiles and m.bwd_pre == (2 if pre == "3" else 0)
    _one("fused e" + pre, "prodLDA", 64, 67, 3, 256, (50,), V=5000, expect=expect)


def test_f_sparse_win_tiles(monkeypatch):
    monkeypatch.setenv("GFEDNTM_WIN_SPARSE", "1")

    def expect(e):
        assert _flags(e) & STAGE_WIN_SPARSE
    _one("fused f", "prodLDA", 32, 63, 31, 20, H2, expect=expect)


def test_g_one_row_batch():
    _one("fused g", "prodLDA", 16, 33, 1, 20, H2)


def test_h_neurallda():
    def expect(e):
        assert e._m.kind == abi.KIND_LDA and abi.PH_LDA_BETA_BWD in e.phases()
    _one("fused h", "LDA", 16, 37, 5, 20, H2, expect=expect, scaled=True)


@pytest.mark.parametrize("forced", [False, True])
def test_j_combined_ctx_kernels(monkeypatch, forced):
    """adapt_bert's Adam in ctx_bwd's epilogue, on both shapes of the kernel."""
    if forced:
        monkeypatch.setenv("GFEDNTM_CTX_FULL", "1")
        monkeypatch.setenv("GFEDNTM_CTX_BWDPP", "1")

    def expect(e):
        assert e._m.ctx_fused == 1 and abi.PH_CTXF_FWD in e.phases() and abi.PH_CTXF_BWD in e.phases()
        assert bool(_flags(e) & STAGE_CTX_FULL) == forced
        assert bool(_flags(e) & STAGE_CTX_BWDPP) == forced
    _one("fused j" + ("-full" if forced else ""), "combined", 16, 35, 3, 20, H2, expect=expect,
         scaled=not forced)


def test_k_zeroshot_dense_input_layer():
    def expect(e):
        assert e._m.ctx_fused == 2
    _one("fused k", "zeroshot", 16, 35, 3, 20, H2, expect=expect)


def test_l_large_batch_beta_adam_in_the_backward():
    """The large-batch plan as production runs it: beta's Adam in the MFMA backward's epilogue
    (lb_fused & 4), the generic optimizer kernel for the rest."""
    def expect(e):
        assert e.large_batch and e.bmax == 256 and _flags(e) & STAGE_LB
        assert e._m.lb_fused & 4 and abi.PH_ADAM in e.phases()
    _one("fused l-prodLDA", "prodLDA", 256, 259, 3, 50, (50, 50), V=3001, expect=expect)


# ---------------------------------------------------------------- (b) one batched launch
def _clients(kind, B, K, H, V, docs, scaled, C=20):
    """M engines with their own seeds, corpora (edge_csr, checked) and plans, bound; the
    number of steps: one epoch of the shortest client plus two."""
    n_steps = min(-(-n // B) for n in docs) + 2
    total = float(sum(docs))
    tms, datas, plans, scales = [], [], [], []
    for i, n_docs in enumerate(docs):
        torch.manual_seed(10 + i)
        kw = dict(input_size=V, n_components=K, hidden_sizes=H, batch_size=B, verbose=False,
                  device="cuda", backend="fused")
        tm = (CombinedTM(contextual_size=C, model_type="prodLDA", **kw) if kind == "combined"
              else AVITM(model_type=kind, **kw))
        assert tm.backend == "fused" and tm.engine.update_mode == UPDATE_FUSED
        plan = BatchPlan.build(n_docs, B, n_steps, seed=i)
        s_partial = -(-n_docs // B) - 1
        assert s_partial < n_steps and int(plan.size[s_partial]) == n_docs % B
        X, marks = edge_csr(n_docs, V, 40, plan, s_partial, seed=1 + i)
        check_edges(X, marks, plan, s_partial, n_steps)
        ctx = None
        if kind == "combined":
            ctx = np.random.default_rng(2 + i).standard_normal((n_docs, C)).astype(np.float32)
        data = DeviceCSR(X, "cuda", contextual=ctx)
        w = n_docs / total if scaled else None
        tm.engine.set_fedavg_scale(w)
        tm.engine.bind_data(data, plan)
        tms.append(tm), datas.append(data), plans.append(plan), scales.append(w)
    assert len({tm.engine.seed for tm in tms}) == len(tms)
    # within one launch: a partial batch next to a full one, or epochs of different lengths
    assert any(len({int(p.size[s]) for p in plans}) > 1 for s in range(n_steps))
    return tms, datas, plans, scales, n_steps


def _batched(case, kind, B, K, H, V, docs, scaled, expect):
    tms, datas, plans, scales, n_steps = _clients(kind, B, K, H, V, docs, scaled)
    engines = [tm.engine for tm in tms]
    for e in engines:
        e.prepare_external_capture()
    bs = BatchedSteps(engines)
    bs.prepare()
    expect(bs, int(bs._host.stage_flags))
    assert bs.plan.startswith("%d clients per launch" % len(docs))
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        bs.launch()
    return walk_fused(tms, datas, plans, n_steps, case, fed_scales=scales, launch=g.replay)


POST_BITS = STAGE_POST_ROWS2 | STAGE_POST_JOINT | STAGE_POST_ROWS4


def test_b1_eight_wave_backward_six_wave_win_update(monkeypatch):
    """prodlda_bwd8_kernel and gfk_win_update_k<512, true, 6>; 129 and 70 documents at B = 64:
    batches of (64, 64), (64, 6), (1, 64), (64, 6), with the pre-scales n_i / sum n."""
    monkeypatch.setenv("GFEDNTM_BWD_WAVES", "8")
    monkeypatch.setenv("GFEDNTM_WIN_WAVES", "6")

    def expect(bs, fl):
        assert fl & STAGE_BWD_BATCH8 and fl & STAGE_WIN_BATCH8 and fl & STAGE_WIN_WAVES6
        assert bs.plan.endswith("prodlda_bwd 8 waves; win_update 8-wave tiles, 6 waves per SIMD")
    _batched("batched B1", "prodLDA", 64, 50, (50, 50), 200, (129, 70), True, expect)


def test_b2_sixteen_wave_backward_eight_wave_win_update_two_joint_rows(monkeypatch):
    """One partial k tile and one partial vocabulary tile (K = 16, V = 40); the 65-document
    client's last batch is one row."""
    monkeypatch.setenv("GFEDNTM_BWD_WAVES", "16")
    monkeypatch.setenv("GFEDNTM_WIN_WAVES", "8")
    monkeypatch.setenv("GFEDNTM_POST_ROWS", "2")

    def expect(bs, fl):
        assert fl & STAGE_WIN_BATCH8 and not fl & STAGE_WIN_WAVES6 and not fl & STAGE_BWD_BATCH8
        assert fl & POST_BITS == STAGE_POST_ROWS2 | STAGE_POST_JOINT
        assert bs.plan.endswith("prodlda_bwd 16 waves; win_update 8-wave tiles, 8 waves per SIMD")
    _batched("batched B2", "prodLDA", 64, 16, (16, 16), 40, (129, 65), False, expect)


def test_b3_four_joint_rows_no_full_batch(monkeypatch):
    """All four k tiles, a last vocabulary tile of 9 columns, four rows per post_bwd workgroup;
    70 and 40 documents: the second client never fills a batch."""
    monkeypatch.setenv("GFEDNTM_BWD_WAVES", "8")
    monkeypatch.setenv("GFEDNTM_WIN_WAVES", "6")
    monkeypatch.setenv("GFEDNTM_POST_ROWS", "4")

    def expect(bs, fl):
        assert fl & STAGE_BWD_BATCH8 and fl & STAGE_WIN_WAVES6 and fl & STAGE_WIN_BATCH8
        assert fl & POST_BITS == POST_BITS
    _batched("batched B3", "prodLDA", 64, 64, (64, 64), 201, (70, 40), False, expect)


def test_b4_three_clients_serial_row_pairs(monkeypatch):
    """Three clients; the 66-document one has a two-row batch inside the launch."""
    monkeypatch.setenv("GFEDNTM_POST_ROWS", "serial2")

    def expect(bs, fl):
        assert fl & POST_BITS == STAGE_POST_ROWS2
    _batched("batched B4", "prodLDA", 64, 50, (50, 50), 200, (70, 66, 129), False, expect)


def test_b5_eight_clients_strip_fill_folded_posterior():
    """Eight clients' strip forwards in one round of the CUs: two tiles per workgroup, the
    posterior folded in by the launch (the engines' own plan keeps post_fwd).  V is the
    smallest at which 8 n_tiles exceeds the CU count: 2100 on the 256 CUs of an MI355X."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    V = 64 * (cus // 8) + 52
    docs = tuple(37 + 2 * i for i in range(8))

    def expect(bs, fl):
        own = bs.engines[0]._m
        assert own.stage_flags & STAGE_FWD_STRIP and not own.stage_flags & STAGE_FWD_POSTFOLD
        assert 8 * own.n_tiles > cus and bs._host.n_tiles == own.n_tiles
        assert bs._host.dec_grid == -(-own.n_tiles // 2) < own.n_tiles
        assert fl & STAGE_FWD_POSTFOLD and abi.PH_POST_FWD not in bs._phases
        assert abi.PH_POST_FWD in bs.engines[0].phases()
    _batched("batched B5", "prodLDA", 16, 20, H2, V, docs, True, expect)


def test_b6_neurallda():
    def expect(bs, fl):
        assert bs._host.kind == abi.KIND_LDA and abi.PH_LDA_BETA_BWD in bs._phases
    _batched("batched B6", "LDA", 16, 20, H2, 701, (37, 33), False, expect)


def test_b7_combined():
    def expect(bs, fl):
        assert bs._host.ctx_fused == 1 and bs.wa_final_phase() == abi.PH_CTXF_BWD
    _batched("batched B7", "combined", 16, 20, H2, 701, (35, 38), True, expect)
