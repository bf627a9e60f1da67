"""ctypes mirror of the C ABI in csrc/gfk_common.h and csrc/step.cpp.

Field order and types MUST match the C structs; :func:`declare` checks the
struct sizes against the library's own ``sizeof`` at load time.
"""
from __future__ import annotations

import ctypes as C

MAX_LAYERS = 8
MAX_SEGS = 48
P = C.c_void_p

# activation / model / input codes
ACT_CODES = {"softplus": 0, "relu": 1, "sigmoid": 2, "tanh": 3, "leakyrelu": 4, "elu": 5,
             "selu": 6, "rrelu": 7}
KIND_PRODLDA, KIND_LDA = 0, 1
IN_BOW, IN_COMBINED, IN_CONTEXTUAL = 0, 1, 2

# stage_flags bits of the batched post_bwd (csrc/gfk_common.h GFK_POST_ROWS2 / GFK_POST_JOINT /
# GFK_POST_ROWS4): several rows per workgroup with the batch-level workgroup in row_bwd; the
# rows through each phase together; four rows instead of two (needs both others)
POST_ROWS2 = 1 << 20
POST_JOINT = 1 << 21
POST_ROWS4 = 1 << 22
# GFEDNTM_POST_ROWS value -> those bits (ops/engine.py post_rows_flags)
POST_ROWS_SHAPES = {"serial2": POST_ROWS2, "2": POST_ROWS2 | POST_JOINT,
                    "4": POST_ROWS2 | POST_JOINT | POST_ROWS4}

# stage_flags bit of the batched ProdLDA tile backward in 8-wave workgroups (csrc/gfk_common.h
# GFK_BWD_BATCH8; ops/engine.py bwd_batch8_flag)
BWD_BATCH8 = 1 << 23
# stage_flags bit of the batched win_update's 8-wave dense tiles compiled for 6 waves per SIMD
# (csrc/gfk_common.h GFK_WIN_WAVES6; ops/engine.py win_waves_flag)
WIN_WAVES6 = 1 << 24

# phase ids (csrc/step.cpp GfkPhase)
PH_BATCH_DOCS = 0
PH_ENC_FWD = 1
PH_POST_FWD = 2
PH_PRODLDA_FWD = 3
PH_PRODLDA_LOSS = 4
PH_PRODLDA_BWD = 5
PH_LDA_BETA_FWD = 6
PH_LDA_ROW = 7
PH_POST_BWD = 8
PH_LDA_BETA_BWD = 9
PH_ENC_BWD = 10
PH_ADAM = 11
PH_BATCH_PREP = 12
PH_CTXF_FWD = 13      # CombinedTM contextual forward on the fused kernels (ctx_fwd)
PH_CTXF_BWD = 14      # ... and its backward + adapt_bert updates (ctx_bwd)

# PH_ENC_FWD = enc_in (sparse gather, MLP, heads, random draws), PH_POST_FWD =
# post_fwd (batch-norm, reparameterisation, softmax, KL), PH_POST_BWD = row_bwd +
# post_bwd, PH_ENC_BWD = win_update (W_in tiles, small-tensor gradient tiles,
# fused updates, next-batch prep).  In fused-update mode the optimizer step lives
# in the kernel epilogues; gradient mode appends the generic Adam.
# host-side phases (CTM): the dense contextual GEMMs around the fused kernels,
# issued on the same stream (hipBLASLt through torch) and captured in the same graph
PH_CTX_FWD = 100
PH_CTX_BWD = 101
# host-side phases (multi-GPU): the FedAvg all-reduce of beta (on a side stream,
# overlapping the encoder backward) and of the rest of the shared state
PH_FEDAVG_BETA = 102
PH_FEDAVG_END = 103
# (104 - 106: round 5's split beta / W_in update phases, removed in round 6)
# CombinedTM (fused): adapt_bert's share of the FedAvg forked onto the side stream once
# ctx_bwd has finished it (overlapping win_update), behind beta's
PH_FEDAVG_WA = 107
# the large-batch plan (bmax 256 / 512): ProdLDA's decoder products as hipBLASLt GEMMs on the
# step's stream -- logits = theta_d beta before prodlda_lb_colbn (PH_PRODLDA_FWD), dbeta and
# d theta_d after prodlda_lb_dlogit (PH_PRODLDA_BWD)
PH_LB_GEMM_FWD = 108
PH_LB_GEMM_BWD = 109
# (110 - 111: round 6's in-epilogue FedAvg phases, removed in round 10)
HOST_PHASES = (PH_CTX_FWD, PH_CTX_BWD, PH_FEDAVG_BETA, PH_FEDAVG_END, PH_FEDAVG_WA, PH_LB_GEMM_FWD,
               PH_LB_GEMM_BWD)

PRODLDA_STEP = [PH_ENC_FWD, PH_POST_FWD, PH_PRODLDA_FWD, PH_PRODLDA_LOSS, PH_PRODLDA_BWD,
                PH_POST_BWD, PH_ENC_BWD]
LDA_STEP = [PH_LDA_BETA_FWD, PH_ENC_FWD, PH_POST_FWD, PH_LDA_ROW, PH_POST_BWD, PH_LDA_BETA_BWD,
            PH_ENC_BWD, PH_ADAM]

SEG_ADAM, SEG_SCALE, SEG_KEEP_GRAD = 1, 2, 4


class GfkModel(C.Structure):
    _fields_ = [
        ("bmax", C.c_int32), ("V", C.c_int32), ("K", C.c_int32), ("n_hidden", C.c_int32),
        ("H", C.c_int32 * MAX_LAYERS),
        ("act", C.c_int32), ("kind", C.c_int32), ("input", C.c_int32), ("C", C.c_int32),
        ("L", C.c_int32), ("vb", C.c_int32), ("n_tiles", C.c_int32), ("dec_grid", C.c_int32),
        ("learn_priors", C.c_int32), ("stage_flags", C.c_int32), ("kt", C.c_int32),
        ("scatter_chunks", C.c_int32), ("n_dpart", C.c_int32), ("n_steps", C.c_int32),
        ("drop_enc", C.c_float), ("drop_theta", C.c_float), ("bn_momentum", C.c_float),
        ("bn_eps", C.c_float), ("kl_weight", C.c_float), ("lb_fused", C.c_int32),
        ("seed", C.c_uint64),
        ("prior_mean", P), ("prior_var", P), ("beta", P), ("w_in", P), ("b_in", P),
        ("w_h", P * MAX_LAYERS), ("b_h", P * MAX_LAYERS),
        ("w_mu", P), ("b_mu", P), ("w_s", P), ("b_s", P),
        ("mu_rm", P), ("mu_rv", P), ("s_rm", P), ("s_rv", P), ("beta_rm", P), ("beta_rv", P),
        ("nbt_mu", P), ("nbt_s", P), ("nbt_beta", P),
        ("g_prior_mean", P), ("g_prior_var", P), ("g_beta", P), ("g_w_in", P), ("g_b_in", P),
        ("g_w_h", P * MAX_LAYERS), ("g_b_h", P * MAX_LAYERS),
        ("g_w_mu", P), ("g_b_mu", P), ("g_w_s", P), ("g_b_s", P),
        ("indptr", P), ("indices", P), ("values", P), ("ctx", P),
        ("plan_order", P), ("plan_start", P), ("plan_size", P),
        ("step", P), ("adam_t", P), ("loss_hist", P),
        ("ws_doc", P), ("ws_nb", P), ("ws_z", P * MAX_LAYERS), ("ws_a", P * MAX_LAYERS), ("ws_hd", P), ("ws_mask_h", P),
        ("ws_mu_raw", P), ("ws_ls_raw", P), ("ws_mu", P), ("ws_ls", P), ("ws_bn_rstd", P),
        ("ws_eps", P), ("ws_theta", P), ("ws_mask_t", P), ("ws_thetad", P),
        ("ws_kl", P), ("ws_rl", P), ("ws_lse", P), ("ws_s", P),
        ("ws_zn", P), ("ws_col_rstd", P), ("ws_row_part", P), ("ws_dthetad", P),
        ("ws_dz", P * MAX_LAYERS), ("ws_dmr", P), ("ws_dlr", P),
        ("ws_dmu", P), ("ws_dls", P),
        ("ws_dbsm", P), ("ws_ck", P), ("ws_hctx", P), ("ws_tstart", P), ("ws_erange", P),
        ("ws_next", P), ("dbg", P),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("adam_eps", C.c_float),
        ("weight_decay", C.c_float), ("fed_scale", C.c_float), ("update_mode", C.c_int32),
        ("fed_scale_on", C.c_int32), ("flat_base", P), ("n_shared", C.c_int64),
        ("off_m", C.c_int64), ("off_v", C.c_int64), ("off_g", C.c_int64),
        ("adam_pow", P), ("adam_coef", P), ("ws_dtheta", P),
        ("w_a", P), ("b_a", P), ("ws_actx", P), ("ws_hpart", P),
        ("ctx_fused", C.c_int32), ("ctx_kb", C.c_int32), ("ctx_ckb", C.c_int32),
        ("slot_cap", C.c_int32), ("ws_sidx", P), ("ws_sval", P),
        ("mm_bf16", C.c_int32), ("ctx_parts", C.c_int32),
        ("lab_on", C.c_int32), ("lab_off", C.c_int32), ("labels", P), ("w_cls", P), ("b_cls", P),
        ("ws_lab", P), ("ws_dlab", P), ("ws_ce", P), ("ws_thd", P),
        ("lab_in_enc", C.c_int32), ("bwd_pre", C.c_int32), ("ws_dt", P),
        ("dev", P), ("dev_upd", P), ("n_batch", C.c_int32), ("ldb", C.c_int32),
        ("ctx_bgrid", C.c_int32), ("epoch_stride", C.c_int32), ("ws_colstat", P),
        ("kl_hist", P), ("rl_hist", P),
        ("off_own", C.c_int64),
        ("epoch_idx", P), ("epoch_run", P), ("epoch_loss", P),
    ]


class GfkWJob(C.Structure):
    _fields_ = [("param", P), ("dz", P), ("a", P), ("rows", C.c_int32), ("cols", C.c_int32),
                ("j0", C.c_int32), ("i0", C.c_int32)]


class GfkVJob(C.Structure):
    _fields_ = [("param", P), ("src", P), ("n", C.c_int32), ("pad", C.c_int32)]


MAX_WJOBS, MAX_VJOBS = 40, 16


class GfkUpdate(C.Structure):
    _fields_ = [("n_w", C.c_int32), ("n_v", C.c_int32), ("w", GfkWJob * MAX_WJOBS),
                ("v", GfkVJob * MAX_VJOBS)]


# update rules of the generic optimizer kernel (csrc/gfk_common.h GFK_SOLVER_*)
ADAM_CHUNK = 256      # float4 per workgroup of the generic optimizer kernel (GFK_ADAM_CHUNK)
SOLVER_CODES = {"adam": 0, "sgd": 1, "adagrad": 2, "adadelta": 3, "rmsprop": 4}


class GfkAdam(C.Structure):
    _fields_ = [
        ("p", P), ("g", P), ("m", P), ("v", P),
        ("n_seg", C.c_int32), ("solver", C.c_int32),
        ("seg_start", C.c_int64 * MAX_SEGS), ("seg_end", C.c_int64 * MAX_SEGS),
        ("seg_flags", C.c_int32 * MAX_SEGS),
        ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("weight_decay", C.c_float), ("scale", C.c_float),
        ("t", P), ("coef", P),
        ("seg_first_block", C.c_int32 * MAX_SEGS), ("dbg", P),
    ]


class GfkInfer(C.Structure):
    """theta-inference launch (csrc/infer.hip)."""
    _fields_ = [("indptr", P), ("indices", P), ("values", P), ("hctx", P), ("out", P),
                ("n_docs", C.c_int32), ("n_samples", C.c_int32), ("flags", C.c_int32),
                ("thr", C.c_float), ("seed", C.c_uint64), ("grid", C.c_int32), ("doc0", C.c_int32)]


INFER_POSTPROCESS, INFER_MOMENTS = 1, 2


class GfkScore(C.Structure):
    """held-out scoring launch (csrc/score.hip)."""
    _fields_ = [("indptr", P), ("indices", P), ("values", P), ("moments", P), ("theta", P),
                ("lse_part", P), ("rl_rows", P), ("out", P),
                ("n_docs", C.c_int32), ("n_samples", C.c_int32), ("seed", C.c_uint64),
                ("grid", C.c_int32), ("doc0", C.c_int32), ("max_grid", C.c_int32)]


class GfkScoreX(C.Structure):
    """held-out scoring launch on the NeuralLDA decoder and / or with a label head
    (csrc/score.hip gfk_score_ext): ``s.out`` is a [n_docs, 2] workspace there."""
    _fields_ = [("s", GfkScore), ("labels", P), ("topic_lse", P), ("ce_rows", P), ("out", P),
                ("ncol", C.c_int32), ("reserved", C.c_int32)]


class GfkCooc(C.Structure):
    """word co-occurrence counting launch (csrc/cooc.hip)."""
    _fields_ = [("indptr", P), ("indices", P), ("values", P), ("slot", P), ("bits", P),
                ("counts", P), ("n_docs", C.c_int64), ("bits_words", C.c_int64),
                ("W", C.c_int32), ("V", C.c_int32), ("max_grid", C.c_int32)]


class GfkDss(C.Structure):
    """document similarity score launch (csrc/simscore.hip)."""
    _fields_ = [("a", P), ("b", P), ("part", P), ("out", P),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("n_docs", C.c_int64),
                ("part_len", C.c_int64),
                ("D", C.c_int32), ("Ka", C.c_int32), ("Kb", C.c_int32),
                ("a_f64", C.c_int32), ("b_f64", C.c_int32), ("max_grid", C.c_int32)]


class GfkBc(C.Structure):
    """Bhattacharyya matrix / topic similarity score launch (csrc/simscore.hip)."""
    _fields_ = [("x", P), ("y", P), ("part", P), ("bc", P), ("tss", P),
                ("ldx", C.c_int64), ("ldy", C.c_int64), ("part_len", C.c_int64),
                ("M", C.c_int32), ("N", C.c_int32), ("L", C.c_int32),
                ("x_f64", C.c_int32), ("y_f64", C.c_int32), ("max_grid", C.c_int32)]


class GfkThin(C.Structure):
    """token-wise thinning launch (csrc/thin.hip)."""
    _fields_ = [("indptr", P), ("indices", P), ("values", P), ("theta", P), ("tw", P),
                ("kept", P), ("p_out", P), ("n_kept", P), ("n_rest", P),
                ("kept_ptr", P), ("rest_ptr", P), ("kept_idx", P), ("kept_val", P),
                ("rest_idx", P), ("rest_val", P),
                ("seed", C.c_uint64), ("rate", C.c_float),
                ("n_docs", C.c_int32), ("K", C.c_int32), ("V", C.c_int32), ("ld", C.c_int32),
                ("topic", C.c_int32), ("doc0", C.c_int32), ("pass_", C.c_int32),
                ("max_grid", C.c_int32)]


THIN_COUNT, THIN_COMPACT = 1, 2


class GfkWmdDist(C.Structure):
    """ground distances between two sets of word vectors (csrc/wmd.hip)."""
    _fields_ = [("a", P), ("b", P), ("out", P),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldo", C.c_int64),
                ("Ua", C.c_int32), ("Ub", C.c_int32), ("dim", C.c_int32),
                ("a_f64", C.c_int32), ("b_f64", C.c_int32), ("max_grid", C.c_int32)]


class GfkWmd(C.Structure):
    """batched uniform-mass optimal transport launch (csrc/wmd.hip)."""
    _fields_ = [("dist", P), ("a_off", P), ("a_idx", P), ("b_off", P), ("b_idx", P),
                ("flow", P), ("val", P), ("status", P),
                ("ldd", C.c_int64), ("flow_len", C.c_int64),
                ("Ua", C.c_int32), ("Ub", C.c_int32), ("La", C.c_int32), ("Lb", C.c_int32),
                ("max_a", C.c_int32), ("max_b", C.c_int32), ("cap", C.c_int32),
                ("max_grid", C.c_int32)]


class GfkLda(C.Structure):
    """collapsed Gibbs LDA launch: init / sweep / recount / merge (csrc/gibbs.hip)."""
    _fields_ = [("indptr", P), ("indices", P), ("tok_ptr", P), ("z", P), ("nwk0", P), ("nk0", P),
                ("alpha", P), ("ndk", P), ("inv", P), ("item_lo", P), ("item_hi", P),
                ("item_row", P), ("mrg_word", P), ("mrg_first", P), ("mrg_n", P),
                ("nwk", P), ("part", P),
                ("seed", C.c_uint64), ("beta", C.c_float), ("vbeta", C.c_float),
                ("n_docs", C.c_int32), ("n_items", C.c_int32), ("K", C.c_int32), ("V", C.c_int32),
                ("doc0", C.c_int32), ("sweep", C.c_int32), ("frozen", C.c_int32),
                ("pass_", C.c_int32), ("max_grid", C.c_int32)]


LDA_INIT, LDA_SWEEP, LDA_RECOUNT, LDA_MERGE = 1, 2, 3, 4

# optional entry points: name -> (argtypes, restype)
_EXTRA = {
    "gfk_theta_infer": ([C.POINTER(GfkModel), C.POINTER(GfkInfer), C.c_void_p], C.c_int),
    "gfk_theta_infer_smem": ([C.POINTER(GfkModel)], C.c_size_t),
}


def declare(lib: C.CDLL) -> None:
    lib.gfk_model_struct_size.restype = C.c_size_t
    lib.gfk_adam_struct_size.restype = C.c_size_t
    if lib.gfk_model_struct_size() != C.sizeof(GfkModel):
        raise RuntimeError(f"GfkModel ABI mismatch: C {lib.gfk_model_struct_size()} vs "
                           f"ctypes {C.sizeof(GfkModel)}")
    if lib.gfk_adam_struct_size() != C.sizeof(GfkAdam):
        raise RuntimeError(f"GfkAdam ABI mismatch: C {lib.gfk_adam_struct_size()} vs "
                           f"ctypes {C.sizeof(GfkAdam)}")
    lib.gfk_update_struct_size.restype = C.c_size_t
    if lib.gfk_update_struct_size() != C.sizeof(GfkUpdate):
        raise RuntimeError("GfkUpdate ABI mismatch")
    lib.gfk_setup.argtypes = [C.POINTER(GfkModel)]
    lib.gfk_setup.restype = C.c_int
    lib.gfk_run.argtypes = [C.POINTER(GfkModel), C.POINTER(GfkAdam), C.c_int, C.POINTER(GfkUpdate),
                            C.c_void_p, C.POINTER(C.c_int32), C.c_int]
    lib.gfk_run.restype = C.c_int
    lib.gfk_smem_required.argtypes = [C.POINTER(GfkModel), C.c_int]
    lib.gfk_smem_required.restype = C.c_size_t
    lib.gfk_scale.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    lib.gfk_scale.restype = C.c_int
    lib.gfk_launch_adam.argtypes = [C.POINTER(GfkAdam), C.c_int, C.c_void_p]
    lib.gfk_launch_adam.restype = C.c_int
    lib.gfk_infer_struct_size.restype = C.c_size_t
    if lib.gfk_infer_struct_size() != C.sizeof(GfkInfer):
        raise RuntimeError("GfkInfer ABI mismatch")
    lib.gfk_score_struct_size.restype = C.c_size_t
    if lib.gfk_score_struct_size() != C.sizeof(GfkScore):
        raise RuntimeError("GfkScore ABI mismatch")
    lib.gfk_doc_score.argtypes = [C.POINTER(GfkModel), C.POINTER(GfkScore), C.c_void_p]
    lib.gfk_doc_score.restype = C.c_int
    lib.gfk_doc_score_smem.argtypes = [C.POINTER(GfkModel)]
    lib.gfk_doc_score_smem.restype = C.c_size_t
    lib.gfk_score_vranges.argtypes = [C.POINTER(GfkModel)]
    lib.gfk_score_vranges.restype = C.c_int
    lib.gfk_scorex_struct_size.restype = C.c_size_t
    if lib.gfk_scorex_struct_size() != C.sizeof(GfkScoreX):
        raise RuntimeError("GfkScoreX ABI mismatch")
    lib.gfk_score_ext.argtypes = [C.POINTER(GfkModel), C.POINTER(GfkScoreX), C.c_void_p]
    lib.gfk_score_ext.restype = C.c_int
    lib.gfk_lda_topic_lse.argtypes = [C.POINTER(GfkModel), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.gfk_lda_topic_lse.restype = C.c_int
    lib.gfk_cooc_struct_size.restype = C.c_size_t
    if lib.gfk_cooc_struct_size() != C.sizeof(GfkCooc):
        raise RuntimeError("GfkCooc ABI mismatch")
    lib.gfk_cooc.argtypes = [C.POINTER(GfkCooc), C.c_void_p]
    lib.gfk_cooc.restype = C.c_int
    lib.gfk_cooc_max_words.argtypes = []
    lib.gfk_cooc_max_words.restype = C.c_int
    lib.gfk_dss_struct_size.restype = C.c_size_t
    lib.gfk_bc_struct_size.restype = C.c_size_t
    if lib.gfk_dss_struct_size() != C.sizeof(GfkDss):
        raise RuntimeError("GfkDss ABI mismatch")
    if lib.gfk_bc_struct_size() != C.sizeof(GfkBc):
        raise RuntimeError("GfkBc ABI mismatch")
    lib.gfk_dss.argtypes = [C.POINTER(GfkDss), C.c_void_p]
    lib.gfk_dss.restype = C.c_int
    lib.gfk_bc.argtypes = [C.POINTER(GfkBc), C.c_void_p]
    lib.gfk_bc.restype = C.c_int
    lib.gfk_sim_max_rows.argtypes = []
    lib.gfk_sim_max_rows.restype = C.c_int
    lib.gfk_dss_items.argtypes = [C.c_int64]
    lib.gfk_dss_items.restype = C.c_int64
    lib.gfk_bc_ranges.argtypes = [C.c_int]
    lib.gfk_bc_ranges.restype = C.c_int
    lib.gfk_thin_struct_size.restype = C.c_size_t
    if lib.gfk_thin_struct_size() != C.sizeof(GfkThin):
        raise RuntimeError("GfkThin ABI mismatch")
    lib.gfk_thin.argtypes = [C.POINTER(GfkThin), C.c_void_p]
    lib.gfk_thin.restype = C.c_int
    lib.gfk_thin_max_topics.argtypes = []
    lib.gfk_thin_max_topics.restype = C.c_int
    lib.gfk_wmd_dist_struct_size.restype = C.c_size_t
    lib.gfk_wmd_struct_size.restype = C.c_size_t
    if lib.gfk_wmd_dist_struct_size() != C.sizeof(GfkWmdDist):
        raise RuntimeError("GfkWmdDist ABI mismatch")
    if lib.gfk_wmd_struct_size() != C.sizeof(GfkWmd):
        raise RuntimeError("GfkWmd ABI mismatch")
    lib.gfk_wmd_dist.argtypes = [C.POINTER(GfkWmdDist), C.c_void_p]
    lib.gfk_wmd_dist.restype = C.c_int
    lib.gfk_wmd_solve.argtypes = [C.POINTER(GfkWmd), C.c_void_p]
    lib.gfk_wmd_solve.restype = C.c_int
    lib.gfk_wmd_max_words.argtypes = []
    lib.gfk_wmd_max_words.restype = C.c_int
    lib.gfk_wmd_grid.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int]
    lib.gfk_wmd_grid.restype = C.c_int
    lib.gfk_wmd_flow_len.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.gfk_wmd_flow_len.restype = C.c_int64
    lib.gfk_lda_struct_size.restype = C.c_size_t
    if lib.gfk_lda_struct_size() != C.sizeof(GfkLda):
        raise RuntimeError("GfkLda ABI mismatch")
    lib.gfk_lda.argtypes = [C.POINTER(GfkLda), C.c_void_p]
    lib.gfk_lda.restype = C.c_int
    lib.gfk_lda_max_topics.argtypes = []
    lib.gfk_lda_max_topics.restype = C.c_int
    lib.gfk_lda_max_doc_tokens.argtypes = []
    lib.gfk_lda_max_doc_tokens.restype = C.c_int
    for name, args in _EXTRA.items():
        if hasattr(lib, name):
            f = getattr(lib, name)
            f.argtypes, f.restype = args


def phase_array(phases):
    arr = (C.c_int32 * len(phases))(*phases)
    return arr, len(phases)
