"""The launch plan of a fused step: which stage bits, grids, d theta_d slabs and kernel shapes
a model's step takes (:func:`plan_step`), and what a batched launch of M clients changes
(:func:`plan_batched`).

The plan is a function of numbers only -- the descriptor's value fields (:func:`fill_shape`),
the CU count, the knobs (:class:`Knobs`), the solver, two facts about the flat layout and the
LDS sizes the kernel library computes on the host (``gfk_smem_required``) -- so it runs
without a GPU: tests/test_plan_golden.py replays tests/golden/step_plans.json through it.
Neither entry point touches the device, the environment or ``gfk_setup``; ops/engine.py reads
the knobs (:meth:`Knobs.from_env`), binds pointers, allocates and uploads.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, fields
from typing import Dict, List, NamedTuple, Optional

from . import kernel_abi as abi

BMAX_CHOICES = (16, 32, 64, 128, 256, 512)
# batch sizes above this run the large-batch plan (csrc/gfk_common.h GFK_LB)
LB_MIN_BMAX = 256
LDS_LIMIT = 160 * 1024
VB = 64
# stage_flags plans, fastest first: bit 0 = MLP weights staged in LDS (enc_in,
# post_bwd); bit 1 = the posterior kernels read the [B, K] batch matrices from L2
# instead of staging them (large K).  Plan 3 (weights staged, batch matrices from L2)
# is the large-K plan: the head weights [K, H] feed post_bwd's GEMVs from LDS instead
# of one dependent L2 round trip per pass
STAGE_PLANS = (1, 0, 3, 2)
STAGE_FWD_STRIP = 4               # bit 2: ProdLDA strip forward (csrc/prodlda.hip)
STAGE_WIN_SPARSE = 16             # bit 4: sparse W_in tiles (csrc/update.hip win_tile_sparse)
STAGE_CTX_FULL = 32               # bit 5: CombinedTM forward, one workgroup per tile (csrc/ctx.hip)
STAGE_WIN_BATCH8 = 512            # bit 9: batched launches: win_update's 8-wave tile shape
STAGE_CTX_BWDPP = 4096            # bit 12: CombinedTM backward, persistent pipelined shape (csrc/ctx.hip)
STAGE_CTX_RS = 32768              # bit 15: CombinedTM forward, Wa register-streamed (csrc/ctx.hip)
STAGE_FWD_POSTFOLD = 65536        # bit 16: the strip forward computes post_fwd (csrc/prodlda.hip FP)
STAGE_LB = 524288                 # bit 19: the large-batch plan (bmax 256 / 512, csrc/gfk_common.h)
STAGE_POST_ROWS2 = abi.POST_ROWS2  # bit 20: batched post_bwd, two rows per workgroup; its batch-level
                                   #         workgroup in row_bwd (csrc/posterior.hip)
STAGE_POST_JOINT = abi.POST_JOINT  # bit 21: ... the rows through each phase together (with bit 20)
STAGE_POST_ROWS4 = abi.POST_ROWS4  # bit 22: ... four rows per workgroup (with bits 20 and 21)
STAGE_BWD_BATCH8 = abi.BWD_BATCH8  # bit 23: batched ProdLDA tile backward, 8-wave workgroups, three per CU
STAGE_WIN_WAVES6 = abi.WIN_WAVES6  # bit 24: batched win_update (with bit 9), 6 waves per SIMD, three per CU
# the LDS one of a CU's three 8-wave backward workgroups may take (csrc/prodlda.hip BWD8_LDS)
BWD8_LDS = LDS_LIMIT // 3
# ... and one of its three 6-waves-per-SIMD win_update workgroups
WIN6_LDS = LDS_LIMIT // 3
# the shape GFEDNTM_POST_ROWS=auto takes where bit 20 applies (a key of abi.POST_ROWS_SHAPES):
# the headline's interleaved A/B, 8 clients K = 50 (profiles/r7/ab_post_rows.txt): serial2
# 0.1176 ms per round, two joint rows 0.1159, four 0.1193
POST_ROWS_AUTO = "2"
# (removed in round 6, measured not faster: bits 3 / 8 the strip forward's 8-wave whole-block
# prefetch vs its ring (now the only variant), bit 6 the plain rolling prefetch, 7 the split W_in update, 10 the sparse tile's register second moment
# as a knob, 11 / 13 the LDS-DMA balanced CombinedTM forwards, 14 the persistent Wc update,
# 17 the moved batch-level workgroup on its own, 18 the one-range backward walking tiles)

UPDATE_GRAD, UPDATE_FUSED = 0, 1


@dataclass(frozen=True)
class Knobs:
    """The plan knobs: field ``x`` is GFEDNTM_X, its default the value an unset variable
    means (docs/DESIGN.md "Stage bits and knobs").  Read once per plan (:meth:`from_env`):
    where FusedEngine fills its descriptor, and at every BatchedSteps refresh."""
    fwd_strip: str = "auto"
    postfold: str = "auto"
    bwd_pre: str = "3"
    ctx_full: str = "auto"
    ctx_rs: str = "1"
    ctx_bwdpp: str = "auto"
    win_sparse: str = "auto"
    lb_gemm: str = "0"
    batch_strip: str = "fill"
    post_rows: str = "auto"
    bwd_waves: str = "auto"
    win_waves: str = "auto"

    @classmethod
    def from_env(cls, env=None) -> "Knobs":
        env = os.environ if env is None else env
        return cls(**{f.name: env.get("GFEDNTM_" + f.name.upper(), f.default) for f in fields(cls)})


def post_rows_flags(n_clients: int, bmax: int, cus: int, knob: str = "auto") -> int:
    """stage_flags bits of a batched launch's post_bwd shape (GFEDNTM_POST_ROWS).

    ``auto``: where M clients' bmax + 1 one-row workgroups exceed one round of the CUs, the
    shape POST_ROWS_AUTO; else none (the one-row shape).  ``serial2`` / ``2`` / ``4`` force
    that shape on every launch of M > 1 clients, whatever the CU count."""
    if n_clients < 2:
        return 0
    if knob == "auto":
        return abi.POST_ROWS_SHAPES[POST_ROWS_AUTO] if n_clients * (bmax + 1) > cus else 0
    if knob not in abi.POST_ROWS_SHAPES:
        raise ValueError(f"GFEDNTM_POST_ROWS={knob!r}: expected auto, serial2, 2 or 4")
    return abi.POST_ROWS_SHAPES[knob]


def _splits_k(K: int) -> bool:
    """K has the four k tiles the k-range backward splits."""
    return -(-K // 16) >= 4


def bwd_kq(n_tiles: int, n_dpart: int, K: int) -> int:
    """k ranges of ProdLDA's tile backward (csrc/prodlda.hip bwd_kq)."""
    return 4 if n_dpart < n_tiles and _splits_k(K) else 1


def bwd8_lds_bytes(bmax: int, K: int, kt: int) -> int:
    """Dynamic LDS of the 8-wave tile backward (csrc/prodlda.hip bwd8_smem): theta_d, the
    region of the logit tile and then the beta block, the logit gradient, lse / S / rstd."""
    kpq = -(-K // 16) * 16
    return 4 * (bmax * kt + max(bmax * VB, kpq * 66) + bmax * 66 + 2 * bmax + VB)


def bwd_batch8_flag(n_clients: int, n_tiles: int, cus: int, *, bmax: int, K: int, bf16: bool,
                    kq: int, bwd_pre: int, lds_bytes: int, knob: str = "auto") -> int:
    """stage_flags bit of a batched launch's ProdLDA tile backward (GFEDNTM_BWD_WAVES).

    The 8-wave instance exists for the one-range tile backward (``kq`` = 1 -- 0 where the
    model runs no tile backward at all --, no precomputed logit gradient) at bmax = 64,
    K <= 64, fp32, within a third of a CU's LDS.  ``auto``: where M clients' tiles are more
    than two 16-wave workgroups per CU hold at once and at most the three 8-wave ones do
    (2 CUs < M n_tiles <= 3 CUs: one round instead of two).  ``8`` / ``16`` force the shape
    on every launch of M > 1 clients; ``8`` without an instance is an error."""
    if knob not in ("auto", "16", "8"):
        raise ValueError(f"GFEDNTM_BWD_WAVES={knob!r}: expected auto, 16 or 8")
    if n_clients < 2 or knob == "16":
        return 0
    exists = (kq == 1 and not bwd_pre and bmax == 64 and K <= 64 and not bf16
              and lds_bytes <= BWD8_LDS)
    if knob == "8":
        if not exists:
            raise RuntimeError("GFEDNTM_BWD_WAVES=8: no 8-wave tile backward for this launch "
                               "(one-range fp32 tile backward, bmax 64, K <= 64, LDS <= %d B)" % BWD8_LDS)
        return STAGE_BWD_BATCH8
    return STAGE_BWD_BATCH8 if exists and 2 * cus < n_clients * n_tiles <= 3 * cus else 0


def win_waves_flag(n_clients: int, n_wg: int, cus: int, *, dense: bool, batch8: bool, fused: bool,
                   H0: int, lds_bytes: int, knob: str = "auto") -> int:
    """stage_flags bits of a batched launch's win_update register budget (GFEDNTM_WIN_WAVES).

    The 8-wave dense tile kernel (stage bit 9) is compiled for 8 waves per SIMD (64 VGPRs,
    which it exceeds: it spills) and, as a second instance (bit 24), for 6 (80 VGPRs, three
    workgroups per CU).  That instance exists for launches of M > 1 clients whose W_in
    gradient runs as dense tiles (``dense``: no sparse tiles, not the large-batch plan), with
    fused updates, H0 <= 64, within a third of a CU's LDS.  ``n_wg``: a client's workgroups
    (tiles, contextual tiles, weight and vector jobs, the next-batch workgroup).  ``auto``:
    bit 24 where the launch takes the 8-wave shape anyway (``batch8``) and three workgroups
    per CU hold every client's at once (M n_wg <= 3 CUs), so the lower occupancy costs no
    second round.  ``6`` / ``8`` force the 8-wave shape at that budget on every launch of
    M > 1 clients with dense tiles (bit 9, and bit 24 for ``6``); ``6`` without an instance
    is an error."""
    if knob not in ("auto", "8", "6"):
        raise ValueError(f"GFEDNTM_WIN_WAVES={knob!r}: expected auto, 8 or 6")
    if n_clients < 2:
        return 0
    exists = bool(dense) and bool(fused) and H0 <= 64 and lds_bytes <= WIN6_LDS
    if knob == "8":
        return STAGE_WIN_BATCH8 if dense else 0
    if knob == "6":
        if not exists:
            raise RuntimeError("GFEDNTM_WIN_WAVES=6: no 6-waves-per-SIMD win_update for this launch "
                               "(dense W_in tiles, fused updates, H0 <= 64, LDS <= %d B)" % WIN6_LDS)
        return STAGE_WIN_BATCH8 | STAGE_WIN_WAVES6
    return STAGE_WIN_WAVES6 if exists and batch8 and n_clients * n_wg <= 3 * cus else 0


def engine_bmax(tm) -> int:
    """Rows the engine's workspaces are sized for: the batch size rounded up to a kernel
    instance.  (K > 256 runs the large-batch plan at the batch's own size since round 6;
    round 5 padded it to 256 rows.)"""
    return next(x for x in BMAX_CHOICES if x >= tm.batch_size)


def uses_large_batch_plan(tm, bmax: int) -> bool:
    """The large-batch plan (csrc/gfk_common.h GFK_LB): 256 / 512 rows, or K > 256 (its
    posterior / decoder shapes take K <= 512) at any batch size."""
    return bmax >= LB_MIN_BMAX or tm.n_components > 256


def theta_stride(K: int) -> int:
    """Row stride of the dropped-out theta workspace: K rounded up to 2 x odd, so the
    decoder MFMAs' A-role reads (16 rows x 2 k per half-wave, ds_read_b32: bank =
    dword % 32) land on 32 distinct banks (B * kt stays a multiple of 4 for LDS-DMA)."""
    kt = -(-K // 2) * 2
    return kt + 2 if (kt // 2) % 2 == 0 else kt


# beta rows padded to whole 64-column tiles (256 B) from this vocabulary size on
# (utils/flat.py): the large-V kernels' RMW tiles never split a cache line with another
# tile, and a tile's columns past V are row padding (prodlda_bwd_pipe_kernel stores there)
BETA_PAD_MIN_V = 8192
BETA_PAD = 64                     # whole 64-column tiles (the pipelined backward's stores rely on it)


def beta_ld(V: int) -> int:
    """beta's row stride in the fused engine's flat layout."""
    return -(-V // BETA_PAD) * BETA_PAD if V >= BETA_PAD_MIN_V else V


def fill_shape(m: "abi.GfkModel", tm, bmax: int, ldb: Optional[int] = None) -> "abi.GfkModel":
    """The descriptor's shape fields from a model's configuration: what the plan and the
    kernel library's LDS sizes read.  ``ldb``: beta's row stride in the flat layout (default:
    the stride the fused layout gives it)."""
    hs = list(tm.hidden_sizes)
    m.bmax, m.V, m.K, m.n_hidden = bmax, tm.input_size, tm.n_components, len(hs)
    m.ldb = beta_ld(m.V) if ldb is None else ldb
    for i, h in enumerate(hs):
        m.H[i] = h
    m.act = abi.ACT_CODES[tm.activation]
    m.mm_bf16 = int(getattr(tm, "matmul_dtype", "fp32") == "bf16")
    m.kind = abi.KIND_PRODLDA if tm.model_type.lower() == "prodlda" else abi.KIND_LDA
    if tm.kind == "ctm":
        m.input = abi.IN_COMBINED if tm.inference_type == "combined" else abi.IN_CONTEXTUAL
        m.C = tm.contextual_size
    else:
        m.input = abi.IN_BOW
    # CTM label head: the labels are the last L inputs of input_layer (CombinedTM
    # [BoW | adapted | labels], ZeroShotTM [contextual | labels])
    m.L = int(getattr(tm, "label_size", 0) or 0)
    m.lab_on = int(m.L > 0)
    if m.lab_on:
        m.lab_off = 2 * tm.input_size if m.input == abi.IN_COMBINED else m.C
    m.vb = VB
    m.n_tiles = -(-m.V // VB)
    m.learn_priors = int(tm.learn_priors)
    m.kt = theta_stride(m.K)
    m.n_dpart = m.n_tiles if m.kind == abi.KIND_PRODLDA else 1
    return m


# ---------------------------------------------------------------------------- predicates
def four_k_ranges(m) -> bool:
    """ProdLDA's backward runs the persistent 4-k-range shape."""
    return bwd_kq(m.n_tiles, m.n_dpart, m.K) == 4


def bwd_pipelined(m) -> bool:
    """... as the software-pipelined kernel (csrc/prodlda.hip bwd_pipe): fp32 operands in
    both its GEMMs, 32-bit buffer offsets into beta, whole 64-column beta rows."""
    return (four_k_ranges(m) and m.bwd_pre == 3 and m.bmax == 64 and m.ldb % 64 == 0
            and m.K * m.ldb * 4 < 0x7FFF0000)


def win_dense(m) -> bool:
    """W_in's gradient runs as dense x^T MFMA tiles (no sparse tiles, not the large-batch plan)."""
    return not m.stage_flags & (STAGE_WIN_SPARSE | STAGE_LB) and m.bmax <= 128


def lb_library_gemms(m) -> bool:
    """The large-batch plan with a decoder product on library GEMMs: its [B, ldb] logit /
    logit-gradient matrix lives in the workspace."""
    return bool(m.stage_flags & STAGE_LB) and (m.lb_fused & 3) != 3


def ctx_gemm_dtype(m) -> Optional[str]:
    """Operand precision of CombinedTM's contextual GEMMs (adapt_bert and its input-layer
    term) in the forward: "bf16" where matmul_dtype = "bf16" runs the register-streamed
    kernel (csrc/ctx.hip gfk_ctx_fwd_rs_k<BF>), else "fp32"; None without them."""
    if m.ctx_fused != 1:
        return None
    rs = STAGE_CTX_FULL | STAGE_CTX_RS
    return "bf16" if m.mm_bf16 and (m.stage_flags & rs) == rs else "fp32"


def gemm_dtypes(m) -> Dict[str, Optional[str]]:
    """Operand precision of each GEMM of the step, as the launchers choose it (read-only; it
    restates csrc/prodlda.hip gfk_launch_prodlda_fwd / _bwd, csrc/neurallda.hip and
    ``ctx_gemm_dtype``): "dec_fwd" (ProdLDA theta_d beta; NeuralLDA theta_d beta_sm),
    "dthetad" (ProdLDA dlogit beta^T, both operands; NeuralLDA g beta_sm^T, beta_sm only),
    "dbeta" (ProdLDA theta_d^T dlogit; NeuralLDA g^T theta_d), "ctx_a" / "ctx_z0"
    (CombinedTM's x_ctx Wa^T and A Wc^T; None without them).  matmul_dtype = "bf16" rounds
    them all except: the pipelined ProdLDA backward keeps fp32 operands in both its GEMMs;
    the large-batch ProdLDA plan has no bf16 instance at all (NeuralLDA's kernels read
    mm_bf16 themselves, at any batch size); the contextual GEMMs round only in the
    register-streamed forward."""
    prod = m.kind == abi.KIND_PRODLDA
    on = bool(m.mm_bf16) and not (prod and m.stage_flags & STAGE_LB)
    bwd = on and not (prod and bwd_pipelined(m))
    name = lambda b: "bf16" if b else "fp32"  # noqa: E731
    ctx = ctx_gemm_dtype(m)
    return {"dec_fwd": name(on), "dthetad": name(bwd), "dbeta": name(bwd),
            "ctx_a": ctx, "ctx_z0": ctx}


def launch_plan(m, update_mode: int) -> str:
    """The launch plan in one phrase (recorded in bench / metrics records)."""
    if m.stage_flags & STAGE_LB:
        if m.kind == abi.KIND_PRODLDA and lb_library_gemms(m):
            return ("large-batch: HIP kernels + hipBLASLt decoder GEMMs"
                    + (" (backward)" if m.lb_fused else "") + ", gradient mode")
        return "large-batch: HIP kernels, gradient mode"
    return "fused kernels" + (" (fused optimizer epilogues)" if update_mode == UPDATE_FUSED else "")


def step_phases(m, update_mode: int) -> List[int]:
    """The phases of one local step (csrc/step.cpp GfkPhase), without the FedAvg hooks."""
    adam = [abi.PH_ADAM] if update_mode == UPDATE_GRAD else []
    if m.kind == abi.KIND_LDA:
        ph = [p for p in abi.LDA_STEP if p != abi.PH_ADAM] + adam
    else:
        ph = abi.PRODLDA_STEP + adam
        if m.stage_flags & STAGE_LB:            # the decoder's GEMMs around its kernels
            if not m.lb_fused & 1:
                ph.insert(ph.index(abi.PH_PRODLDA_FWD), abi.PH_LB_GEMM_FWD)
            if not m.lb_fused & 2:
                ph.insert(ph.index(abi.PH_PRODLDA_BWD) + 1, abi.PH_LB_GEMM_BWD)
        if m.stage_flags & STAGE_FWD_POSTFOLD:
            ph.remove(abi.PH_POST_FWD)          # computed by the strip forward
    if m.ctx_fused == 1:
        ph.insert(ph.index(abi.PH_ENC_FWD), abi.PH_CTXF_FWD)
        ph.insert(ph.index(abi.PH_ENC_BWD), abi.PH_CTXF_BWD)
    elif m.input != abi.IN_BOW and not m.ctx_fused:     # the contextual path on host GEMMs
        ph.insert(ph.index(abi.PH_ENC_FWD), abi.PH_CTX_FWD)
        ph.insert(ph.index(abi.PH_ENC_BWD) + 1, abi.PH_CTX_BWD)
    return ph


# ---------------------------------------------------------------------------- LDS
def lds_need(lib, m) -> int:
    """Largest dynamic LDS any kernel of this model's step needs under the descriptor's
    current plan, as computed by the kernel library itself: the model's decoder family, the
    posterior kernels, win_update, enc_in, the fused contextual kernels (0 without them)."""
    which = (0, 1) if m.kind == abi.KIND_PRODLDA else (2, 3)
    return int(max(lib.gfk_smem_required(C.byref(m), w) for w in which + (4, 5, 7, 8)))


def fit_stage_plan(lib, m, plans=STAGE_PLANS) -> int:
    """Set ``m.stage_flags`` to the first of ``plans`` that fits the 160 KiB of LDS and
    return its need; where none fits, the last one's (> LDS_LIMIT)."""
    for flags in plans:
        m.stage_flags = flags
        need = lds_need(lib, m)
        if need <= LDS_LIMIT:
            break
    return need


def _force_k_split(lib, m) -> bool:
    """ProdLDA backward at large K with few vocab tiles: the one-range shape (a workgroup
    per tile, all K topics of theta_d and the beta tile in LDS) exceeds the LDS at
    K = 256, B >= 64.  Then use the 4-k-range shape anyway (persistent, n_dpart < n_tiles
    slabs; ~71 KB at K = 256).  Returns True when it set n_dpart so."""
    if m.kind != abi.KIND_PRODLDA or m.n_tiles < 2 or not _splits_k(m.K):
        return False
    m.n_dpart = m.n_tiles
    if lib.gfk_smem_required(C.byref(m), 1) <= LDS_LIMIT:
        return False
    m.n_dpart = m.n_tiles - 1
    return True


def lds_required(lib, tm, bmax: int) -> int:
    """Largest dynamic LDS any fused kernel needs for this model under the last-resort plan
    (weights unstaged), as computed by the kernel library itself.  The contextual kernels do
    not count (the engine falls back from them), and, as ever, neither do CombinedTM's
    contextual W_in tile and the label head's rows: the model is sized as its bag-of-words
    part."""
    m = fill_shape(abi.GfkModel(), tm, bmax)
    m.input, m.C, m.L, m.lab_on, m.lab_off = abi.IN_BOW, 0, 0, 0, 0
    if uses_large_batch_plan(tm, bmax):
        need = 0
        for win in (0, STAGE_WIN_SPARSE):        # (either W_in tile shape)
            m.stage_flags, m.n_dpart = 2 | STAGE_LB | win, 1
            need = max(need, lds_need(lib, m))
        return need
    _force_k_split(lib, m)
    # weights unstaged; batch matrices in LDS, then in L2
    return fit_stage_plan(lib, m, tuple(p for p in STAGE_PLANS if not p & 1))


# ---------------------------------------------------------------------------- one engine
class StepPlan(NamedTuple):
    """What :func:`plan_step` decides besides descriptor fields."""
    postfold_ok: bool                 # a batched launch may fold post_fwd into the strip forward
    ctx_fallback: Optional[str]       # why the contextual path runs on host GEMMs, or None


def plan_step(lib, m, cu: int, knobs: Knobs, solver: str, n_total: int,
              wa_aligned: bool = True) -> StepPlan:
    """The launch plan of one engine's step.  ``m``: a descriptor with its shape fields set
    (:func:`fill_shape`); ``cu``: the device's compute units; ``n_total``: the flat buffer's
    floats; ``wa_aligned``: adapt_bert.weight sits on a 16-byte boundary of it.  Sets
    stage_flags, dec_grid, n_dpart, bwd_pre, lb_fused, ctx_fused, ctx_kb, ctx_ckb, ctx_parts
    and ctx_bgrid; ``lib`` is asked for ``gfk_smem_required`` only."""
    ctx_why = _plan_ctx(lib, m, cu, wa_aligned) if m.input != abi.IN_BOW else None
    m.dec_grid = int(min(m.n_tiles, 2 * cu))
    if m.bmax >= LB_MIN_BMAX or m.K > 256:
        _plan_large_batch(lib, m, cu, knobs, solver)
        return StepPlan(False, ctx_why)
    k_split = _force_k_split(lib, m)
    need = fit_stage_plan(lib, m)         # first plan that fits the 160 KiB of LDS
    if need > LDS_LIMIT:
        raise RuntimeError(f"fused step needs {need} B of LDS (> {LDS_LIMIT})")
    postfold_ok = False
    if m.kind == abi.KIND_PRODLDA:
        # persistent decoder forward: one workgroup per resident slot (16-wave
        # workgroups: 2 per CU when the LDS allows), each looping over its vocab
        # tiles with theta_d staged once and its row-LSE partials merged
        sm = lib.gfk_smem_required(C.byref(m), 0)
        m.dec_grid = int(min(m.n_tiles, (2 if 2 * sm <= LDS_LIMIT else 1) * cu))
        # strip forward (prodlda_fwd_strip_kernel, stage_flags bit 2): each wave owns
        # 16 columns x all rows, beta straight into registers, batch norm without
        # barriers.  The default wherever it applies (fp32, B <= 64): interleaved A/B
        # vs the tile kernel (profiles/r2/ab_strip_forward.txt) K=50 headline 0.0583
        # vs 0.0589 ms, K=50 V=28k 0.092 vs 0.101, K=200 V=112k 0.342 vs 0.349, CTM /
        # ZeroShotTM K=100 neutral.  GFEDNTM_FWD_STRIP=0 selects the tile kernel
        # (bf16 GEMMs: the ring variant with v_mfma_f32_16x16x32_bf16, 32-k steps)
        fits = (m.bmax <= 64 and m.K <= 256 and m.K * m.ldb < (1 << 29))
        if fits and knobs.fwd_strip in ("1", "auto"):
            m.stage_flags |= STAGE_FWD_STRIP
            # the rolling prefetch: the next strip's k pair loaded into the registers
            # its MFMAs just consumed, through a ring of <= 13 pairs (K > 104: 128 VGPRs,
            # 16 waves per CU; K = 200 V = 112k forward 39.7 -> 36.5 us, round 0.2794 ->
            # 0.2751 ms).  Rounds 5-6 removed the other strip variants: the plain rolling
            # one, the non-prefetching one and the 8-wave whole-block prefetch, measured
            # slower (profiles/r3, r4, r6/ab_strip_pf_vs_ring.txt)
            m.dec_grid = int(min(m.n_tiles, cu))
            # the batch-coupled posterior (BN of the heads, reparameterisation, softmax,
            # dropout, KL) inside the ring forward's theta_d staging: post_fwd is not
            # launched (K <= 64, no label head; csrc/gfk_common.h gfk_postfold).  Where it
            # pays: batched launches of several clients (BatchedSteps, sim8 strip forward
            # + post_fwd 27.4 -> 20.5 us); for ONE client the redundant per-workgroup
            # statistics lengthen the forward's critical path more than the launch they
            # save (interleaved, one box: 0.0601 vs 0.0597 ms per round,
            # profiles/r5/ab_fold.txt).  GFEDNTM_POSTFOLD=1 forces it here, =0 everywhere
            postfold_ok = bool(m.K <= 64 and not m.lab_on)
            if postfold_ok and knobs.postfold == "1":
                m.stage_flags |= STAGE_FWD_POSTFOLD
        # backward: one workgroup per tile while the tiles fit the resident slots;
        # else persistent, n_dpart d theta_d slabs: with >= 4 k tiles the topics
        # are split over 4 workgroups per slab (csrc/prodlda.hip, 8 waves each, two
        # per CU when their LDS allows), otherwise one 16-wave workgroup per CU
        m.n_dpart = m.n_tiles
        sb = lib.gfk_smem_required(C.byref(m), 1)      # one tile per workgroup
        if m.n_tiles <= (2 if 2 * sb <= LDS_LIMIT else 1) * cu and not k_split:
            m.n_dpart = m.n_tiles
        elif _splits_k(m.K):
            m.n_dpart = min(cu // 2, m.n_tiles - 1)
            if 2 * lib.gfk_smem_required(C.byref(m), 1) > LDS_LIMIT:
                m.n_dpart = min(cu // 4, m.n_tiles - 1)
        else:
            m.n_dpart = cu
        # the persistent k-range backward (4 workgroups per vocab tile) takes its
        # logit-gradient tiles precomputed once per tile by prodlda_dlogit instead of
        # recomputing them in each range workgroup; GFEDNTM_BWD_PRE=0 selects the
        # recomputing variant
        # (2: two per CU; 3, the default: two per CU, software-pipelined -- the next
        # tile's loads in flight during this tile's compute and stores -- where it
        # applies: fp32, B = 64.  Round 6 removed the 80-VGPR three-per-CU shape and the
        # split beta Adam pass, both measured slower: profiles/r2, profiles/r4)
        m.bwd_pre = (int(knobs.bwd_pre) if four_k_ranges(m) and m.bmax <= 64
                     and knobs.bwd_pre in ("2", "3") else 0)
        if m.bwd_pre and not bwd_pipelined(m):
            m.bwd_pre = 2            # two per CU, no register cap
    # CombinedTM at large V: ctx_fwd with all batch rows per vocab tile (each Wa block
    # staged once instead of once per 16-row block); GFEDNTM_CTX_FULL=0 / 1 overrides
    # (matmul_dtype = "bf16": the register-streamed forward at any V -- the variant with
    # bf16 operands on the matrix cores; the other shapes keep fp32 GEMMs)
    if m.ctx_fused == 1 and m.bmax <= 64 and (
            knobs.ctx_full == "1" or (knobs.ctx_full == "auto" and (m.n_tiles > 2 * cu or m.mm_bf16))):
        m.stage_flags |= STAGE_CTX_FULL
        # ... as the register-streamed persistent kernel: one 16-wave workgroup per CU
        # owns an equal range of 16-column units (at most 32: V <= 131k on 256 CUs), Wa
        # streamed from global memory into registers as the MFMA A operand, x_ctx staged
        # once per workgroup in 256-float phases; each workgroup leaves one contextual z0
        # partial (ctx_parts for enc_in).  V = 99k, interleaved: ctx_fwd 134 -> 122 us,
        # round 0.7386 -> 0.7287 ms (profiles/r4/ab_s8).  GFEDNTM_CTX_RS=0 keeps the
        # one-workgroup-per-tile kernel.  (Round 6 removed the LDS-DMA balanced shapes,
        # bits 11 / 13, measured slower than this one.)
        n_units = -(-int(m.V) // 16)
        if (knobs.ctx_rs != "0" and int(m.H[0]) <= 64
                and -(-n_units // min(m.n_tiles, cu)) <= 32
                and m.V * m.C * 4 < (1 << 31) and 4 * n_total < (1 << 31)):
            m.stage_flags |= STAGE_CTX_RS
            m.ctx_parts = int(min(m.n_tiles, cu))
    # CombinedTM backward as one persistent workgroup per CU walking equal ranges of the
    # (tile, C chunk) items with the next item's Wa state in flight (csrc/ctx.hip
    # gfk_ctx_bwd_pp_k); GFEDNTM_CTX_BWDPP=0 keeps the (tile, chunk) grid
    if (m.ctx_fused == 1 and m.bmax <= 64 and int(m.H[0]) <= 64
            and (knobs.ctx_bwdpp == "1" or (knobs.ctx_bwdpp == "auto" and m.n_tiles > 2 * cu))):
        m.stage_flags |= STAGE_CTX_BWDPP
        m.ctx_bgrid = int(cu)
    # W_in tiles as entry lists instead of dense x^T MFMA tiles where a 64-word tile
    # holds few non-zeros (large vocabularies, the 8-wave update shape: more tiles than
    # two rounds of workgroups); GFEDNTM_WIN_SPARSE=0 keeps the dense tiles
    # (fused CombinedTM too: its bag-of-words half as sparse tiles, the contextual half
    # as dense tiles of the same launch -- csrc/update.hip win_tile_ctx; B <= 64)
    comb = m.input == abi.IN_COMBINED and m.ctx_fused == 1 and m.bmax <= 64
    if (m.input == abi.IN_BOW or comb) and int(m.H[0]) <= 64 and m.bmax <= 128 and _win_sparse(m, cu, knobs):
        m.stage_flags |= STAGE_WIN_SPARSE
        # fused CombinedTM: the contextual half (Wc) as dense tiles of the same launch.
        # (Round 6 removed three opt-in variants measured slower: Wc as a persistent
        # kernel -- V = 99k, 0.7389 vs 0.7309 ms; the sparse tile's second moment in
        # registers instead of LDS -- profiles/r3/win_vl/; the split W_in update, the
        # words outside the batch on a side stream -- K=200 V=112k 0.320 vs 0.294 ms,
        # profiles/r3/win_split.md)
    return StepPlan(postfold_ok, ctx_why)


def _win_sparse(m, cu: int, knobs: Knobs) -> bool:
    """GFEDNTM_WIN_SPARSE: 1 / 0, or more tiles than 4 rounds of the CUs."""
    return knobs.win_sparse == "1" or (knobs.win_sparse == "auto" and m.n_tiles > 4 * cu)


def _plan_large_batch(lib, m, cu: int, knobs: Knobs, solver: str):
    """The large-batch plan, 128 < batch_size <= 512 (csrc/gfk_common.h GFK_LB; reference
    avitm.py:84-85 takes any batch_size).  The row-parallel kernels (enc_in, post_fwd,
    row_loss, row_bwd, post_bwd) run as for small batches with the [B, K] batch matrices
    read from L2 (bit 1), W_in's gradient on the sparse tiles (bit 4), the weight jobs and
    NeuralLDA's beta backward in 128-row chunks.  ProdLDA's decoder: logits = theta_d beta,
    dbeta = theta_d^T dlogit and d theta_d = dlogit beta^T are hipBLASLt GEMMs on the step's
    stream (PH_LB_GEMM_FWD / _BWD: at B >= 256 they are large enough to run near the
    matrix cores' fp32 peak) around prodlda_lb_colbn (column batch-norm, BN'ed tiles, row
    sum-exp partials) and prodlda_lb_dlogit (the logit gradient) -- one slab of d theta_d,
    the [B, ldb] logit / logit-gradient matrix in ws["dt"].  Gradient mode: the generic
    optimizer kernel updates every tensor (as the CTM host-GEMM path)."""
    # W_in's gradient: the sparse entry-list tiles where a 64-word tile holds few of the
    # batch's non-zeros (more tiles than 4 rounds of the CUs, as for small batches), else
    # the dense tiles in 128-row chunks (csrc/update.hip win_tile_dense_ch);
    # GFEDNTM_WIN_SPARSE=1 / 0 forces either
    m.stage_flags = 2 | STAGE_LB | (STAGE_WIN_SPARSE if _win_sparse(m, cu, knobs) else 0)
    m.dec_grid = int(min(m.n_tiles, 2 * cu))
    m.n_dpart = 1
    m.bwd_pre = 0
    # ProdLDA's decoder on the matrix cores (csrc/prodlda.hip prodlda_lb_fwd / _bwd) at
    # bmax 256, K <= 208: one 16-wave workgroup per CU, persistent over the tiles, the
    # backward's d theta_d in one slab per workgroup.  Elsewhere (bmax 512, K > 208) and
    # with GFEDNTM_LB_GEMM=1: the library GEMMs around the HIP kernels.
    m.lb_fused = 0
    if m.kind == abi.KIND_PRODLDA and int(m.K) <= 208 and m.bmax == 256 and knobs.lb_gemm != "1":
        # (+ bit 2: beta's Adam step in prodlda_lb_bwd's epilogue -- the generic optimizer
        # pass then skips beta, 80 % of the parameters at K = 200, V = 112k)
        m.lb_fused = 3 | (4 if solver == "adam" else 0)
        m.dec_grid = int(min(m.n_tiles, cu))
        if m.lb_fused & 2:
            m.n_dpart = m.dec_grid
    need = lds_need(lib, m)
    if need > LDS_LIMIT:
        raise RuntimeError(f"large-batch plan needs {need} B of LDS (> {LDS_LIMIT})")


def _plan_ctx(lib, m, cu: int, wa_aligned: bool) -> Optional[str]:
    """Fused CombinedTM contextual kernels (csrc/ctx.hip).  The forward runs one
    workgroup per (vocab tile, 16-row block); the backward splits C into chunks
    of 16k <= 256 floats, enough of them that n_tiles x chunks covers the CUs
    once (one 16-wave workgroup per CU).  Falls back to the host GEMMs when a shape is outside
    the kernels' assumptions (C % 4, H0 <= 512, LDS): returns why, else None."""
    if m.input == abi.IN_CONTEXTUAL:
        # ZeroShotTM: the [C, H0] input layer is gathered densely by enc_in and its
        # gradient + Adam are ceil(C / 64) extra win_update tiles
        m.ctx_fused = 2 if int(m.H[0]) <= 512 else 0
        return None if m.ctx_fused else f"H0 = {int(m.H[0])} > 512"
    Cs = int(m.C)
    k = max(1, min(cu // m.n_tiles, -(-Cs // 16)))      # one round, one workgroup per CU
    m.ctx_ckb = min(256, -(-(-(-Cs // k)) // 16) * 16)
    m.ctx_kb = -(-Cs // m.ctx_ckb)
    m.ctx_fused = 1
    why = [w for ok, w in (
        (lib.gfk_smem_required(C.byref(m), 8) <= LDS_LIMIT, "LDS plan exceeds 160 KiB"),
        (int(m.H[0]) <= 512, f"H0 = {int(m.H[0])} > 512"),
        (Cs % 4 == 0, f"contextual_size = {Cs} is not a multiple of 4"),
        (wa_aligned, "adapt_bert is not 16-byte aligned in the flat buffer")) if not ok]
    if why:
        m.ctx_fused, m.ctx_kb = 0, 0
        return "; ".join(why)
    return None


# ---------------------------------------------------------------------------- M clients
class BatchedPlan(NamedTuple):
    """What a launch of M clients changes in every client's descriptor, and its records."""
    stage_flags: int
    dec_grid: int
    ctx_bgrid: int
    setup_flags: Optional[int]        # stage_flags to call gfk_setup under (new kernels' LDS), or None
    phases: List[int]
    text: str                         # "8 clients per launch; prodlda_bwd 8 waves"


def plan_batched(lib, m, M: int, cu: int, knobs: Knobs, n_w: int, n_v: int, update_mode: int,
                 postfold_ok: bool, phases: List[int]) -> BatchedPlan:
    """The plan of one launch per phase for M clients' steps.  ``m``: one client's descriptor
    as its own plan left it (not changed); ``n_w`` / ``n_v``: its weight and vector jobs;
    ``postfold_ok``: its :class:`StepPlan`'s; ``phases``: its step's phases."""
    mm = abi.GfkModel.from_buffer_copy(bytes(m))
    # the strip forward: M clients' tiles in one launch of 16-wave workgroups (one per
    # CU).  The strips are grid-strided (a workgroup's wave group g takes tiles
    # g grid + x, so any grid works): where M clients' one-tile-per-workgroup grids
    # exceed one round of the CUs, each workgroup takes T whole tiles (one strip per
    # wave), T the FEWEST in 1..4 whose M ceil(n_tiles / T) workgroups still fit one
    # round -- T = 3 at M = 8, V = 4.7k: 192 workgroups of 12 busy waves instead of
    # 144 of 16; past 4 tiles the M clients share one round (dec_grid = CUs / M).
    # NeuralLDA's decoder kernels (beta forward / backward, grid-strided over the
    # tiles) likewise: T tiles per workgroup so the M clients' workgroups fit one
    # round of the CUs -- the backward's theta_d staging is then paid once per T
    # tiles (8 clients, V = 4.7k: 0.1426 -> 0.1407 ms, same bits; one round of two
    # workgroups per CU measured 0.1497, profiles/r6/lda/ab_batch_fill.txt).
    # GFEDNTM_BATCH_STRIP=keep: the engines' own grids (rounds of the CUs).
    if ((mm.stage_flags & STAGE_FWD_STRIP or mm.kind == abi.KIND_LDA)
            and M > 1 and M * mm.dec_grid > cu and knobs.batch_strip != "keep"):
        t = next((t for t in (1, 2, 3, 4) if M * -(-mm.n_tiles // t) <= cu), None)
        mm.dec_grid = -(-mm.n_tiles // t) if t else max(1, cu // M)
    # the posterior folded into the strip forward for M > 1 clients (the engines' own
    # plan keeps post_fwd for one client; GFEDNTM_POSTFOLD=0: never)
    if M > 1 and postfold_ok and mm.stage_flags & STAGE_FWD_STRIP and knobs.postfold != "0":
        mm.stage_flags |= STAGE_FWD_POSTFOLD
    # post_bwd: M clients x (bmax + 1) workgroups of 16 waves with the batch matrices
    # in LDS (~93 KB: one per CU) run in three rounds at M = 8.  Two rows per
    # workgroup (the matrices, weights and column sums staged once for both) and the
    # batch-level workgroup moved into row_bwd: M bmax / 2 workgroups, one round
    # (M (bmax + 1) <= CUs: the one-row shape).  Round 6 removed the opt-in variants
    # measured slower: the matrices read from L2, and the persistent one-range
    # backward walking several tiles (profiles/r5/ab_batch.txt).
    # GFEDNTM_POST_ROWS = auto | serial2 | 2 | 4: the rows of a workgroup one after the
    # other (serial2) or through each phase together (2 / 4 rows, bits 21 / 22; the
    # own-row vectors of all rows in LDS: gfk_setup raises the kernels' limit)
    setup = False
    post = post_rows_flags(M, mm.bmax, cu, knobs.post_rows)
    if post & STAGE_POST_JOINT:
        mm.stage_flags |= post
        if lib.gfk_smem_required(C.byref(mm), 4) > LDS_LIMIT:
            if knobs.post_rows != "auto":
                raise RuntimeError(f"GFEDNTM_POST_ROWS={knobs.post_rows}: the rows' vectors do not fit the LDS")
            mm.stage_flags &= ~(STAGE_POST_JOINT | STAGE_POST_ROWS4)
        else:
            setup = True
    mm.stage_flags |= post & STAGE_POST_ROWS2
    # CombinedTM: M clients' vocabulary tiles in one launch fill the CUs the way one
    # client's do at a large vocabulary, so the batched launch takes that plan -- the
    # forward with all batch rows per tile (each Wa block staged once) and the
    # persistent pipelined backward -- once M n_tiles > 2 CUs (V = 5k, 8 clients:
    # 0.5296 -> 0.5175 / 0.5137 ms each, profiles/r6/ctm_batched/).  The z0 partials
    # keep the per-tile layout (no register-streamed forward here).
    # GFEDNTM_CTX_FULL / GFEDNTM_CTX_BWDPP = 0: the engines' own plan.
    if (M > 1 and mm.ctx_fused == 1 and mm.bmax <= 64 and int(mm.H[0]) <= 64
            and M * mm.n_tiles > 2 * cu):
        if not mm.stage_flags & STAGE_CTX_FULL and knobs.ctx_full == "auto":
            mm.stage_flags |= STAGE_CTX_FULL
            setup = True                 # (the new kernels' dynamic-LDS limit)
        if not mm.stage_flags & STAGE_CTX_BWDPP and knobs.ctx_bwdpp == "auto":
            mm.stage_flags |= STAGE_CTX_BWDPP
            mm.ctx_bgrid = int(cu)
            setup = True
    setup_flags = int(mm.stage_flags) if setup else None
    # win_update: all clients' W_in tiles in one launch -> the 8-wave tile shape once
    # they exceed two rounds of 16-wave workgroups
    if M * (mm.n_tiles + 8) > 2 * cu:
        mm.stage_flags |= STAGE_WIN_BATCH8
    # prodlda_bwd: two 16-wave workgroups share a CU, so 8 clients x 74 tiles run as
    # a round of 64 tiles per XCD and a second one of 10; three 8-wave workgroups
    # per CU hold them all at once.  GFEDNTM_BWD_WAVES = auto | 16 | 8
    tile_bwd = (mm.kind == abi.KIND_PRODLDA and not mm.stage_flags & STAGE_LB
                and abi.PH_PRODLDA_BWD in phases)
    mm.stage_flags |= bwd_batch8_flag(
        M, mm.n_tiles, cu, bmax=mm.bmax, K=mm.K, bf16=bool(mm.mm_bf16),
        kq=bwd_kq(mm.n_tiles, mm.n_dpart, mm.K) if tile_bwd else 0, bwd_pre=mm.bwd_pre,
        lds_bytes=bwd8_lds_bytes(mm.bmax, mm.K, mm.kt), knob=knobs.bwd_waves)
    # win_update's 8-wave tile kernel needs more than the 64 VGPRs of 8 waves per SIMD;
    # at 6 (80 VGPRs) three workgroups share a CU, enough where they hold every
    # client's tiles and jobs at once.  GFEDNTM_WIN_WAVES = auto | 8 | 6
    extra = mm.n_tiles if mm.ctx_fused == 1 else -(-mm.C // VB) if mm.ctx_fused == 2 else 0
    mm.stage_flags |= win_waves_flag(
        M, mm.n_tiles + extra + n_w + n_v + 1, cu, dense=win_dense(mm),
        batch8=bool(mm.stage_flags & STAGE_WIN_BATCH8), fused=update_mode == UPDATE_FUSED,
        H0=int(mm.H[0]), lds_bytes=int(lib.gfk_smem_required(C.byref(mm), 5)),
        knob=knobs.win_waves)
    # the phases of the batched plan: post_fwd out where the launch folds it, back in
    # where the launch dropped the engines' fold
    ph = list(phases)
    folded = bool(mm.stage_flags & STAGE_FWD_POSTFOLD)
    if folded and abi.PH_POST_FWD in ph:
        ph.remove(abi.PH_POST_FWD)
    elif not folded and abi.PH_PRODLDA_FWD in ph and abi.PH_POST_FWD not in ph:
        ph.insert(ph.index(abi.PH_PRODLDA_FWD), abi.PH_POST_FWD)
    # the shapes this launch runs, for records: "8 clients per launch; prodlda_bwd 8 waves"
    text = "%d clients per launch" % M
    if abi.PH_PRODLDA_BWD in ph and not mm.stage_flags & STAGE_LB:
        text += "; prodlda_bwd " + ("8 waves" if mm.stage_flags & STAGE_BWD_BATCH8 else
                                    "k ranges" if four_k_ranges(mm) else "16 waves")
    if mm.stage_flags & STAGE_WIN_BATCH8 and win_dense(mm):
        text += "; win_update 8-wave tiles, %d waves per SIMD" % (
            6 if mm.stage_flags & STAGE_WIN_WAVES6 else 8)
    return BatchedPlan(int(mm.stage_flags), int(mm.dec_grid), int(mm.ctx_bgrid), setup_flags, ph, text)
