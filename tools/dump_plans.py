"""Record the launch plan of every shape the fused step can take: tests/golden/step_plans.json.

For each case of CASES (a model's constructor arguments, the GFEDNTM_* plan knobs, the
number of batched clients) the file holds what the planner is given beyond those -- the CU
count, beta's row stride, the flat buffer's length, whether adapt_bert sits on a 16-byte
boundary, the update job counts -- and what comes out: every value field of the engine's
descriptor (and of the batched launch's), the update mode, the phase lists, the plan strings,
the GEMM operand types, the contextual fallback reason; for a case that raises, the exception.
tests/test_plan_golden.py replays the file through gfedntm_amd/ops/plan.py without a GPU and
through the engines on one.

    python tools/dump_plans.py [out.json]       (on the GPU the file is recorded for)

Constructing an engine launches no step kernel; the largest case allocates about 0.4 GB.
"""
from __future__ import annotations

import ctypes as C
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_plans.json")
KNOBS = ("FWD_STRIP", "POSTFOLD", "BWD_PRE", "CTX_FULL", "CTX_RS", "CTX_BWDPP", "WIN_SPARSE",
         "LB_GEMM", "BATCH_STRIP", "POST_ROWS", "BWD_WAVES", "WIN_WAVES")
# descriptor fields that hold addresses in disguise (distances between allocations)
ADDRESS_FIELDS = ("off_m", "off_v", "off_g", "off_own")


def _case(name, model="avitm", M=0, env=None, **kw):
    kw = {"input_size": 4718, "n_components": 50, "hidden_sizes": (50, 50), "batch_size": 64, **kw}
    return {"name": name, "model": model, "M": M, "env": dict(env or {}), "kw": kw}


def _cases():
    big = dict(input_size=112000, n_components=200)
    out = [
        # ProdLDA, hidden (50, 50), B = 64
        _case("headline"),
        _case("k200_l2", input_size=3000, n_components=200),
        _case("v112k_k200", **big),
        _case("v112k_k200_pre2", env={"BWD_PRE": "2"}, **big),
        _case("v112k_k200_pre0", env={"BWD_PRE": "0"}, **big),
        _case("v112k_k200_pre3", env={"BWD_PRE": "3"}, **big),
        _case("v112k_k48", input_size=112000, n_components=48),
        _case("v112k_k48_dense", env={"WIN_SPARSE": "0"}, input_size=112000, n_components=48),
        _case("v130_k256_ksplit", input_size=130, n_components=256),
        _case("v130_k256_tile_fwd", env={"FWD_STRIP": "0"}, input_size=130, n_components=256),
        _case("v8191", input_size=8191),
        _case("v8192", input_size=8192),
        _case("v33k_two_per_cu", input_size=33000),       # 516 tiles: past two rounds of the CUs
        _case("b16", batch_size=16),
        _case("b32", batch_size=32),
        _case("b128", batch_size=128),
        _case("bf16", matmul_dtype="bf16"),
        _case("bf16_v112k_k200", matmul_dtype="bf16", **big),
        _case("bf16_v112k_k200_pre2", env={"BWD_PRE": "2"}, matmul_dtype="bf16", **big),
        _case("strip0", env={"FWD_STRIP": "0"}),
        _case("strip1", env={"FWD_STRIP": "1"}),
        _case("strip_auto", env={"FWD_STRIP": "auto"}),
        _case("postfold1", env={"POSTFOLD": "1"}),
        _case("postfold1_k65", env={"POSTFOLD": "1"}, n_components=65),
        _case("sparse1", env={"WIN_SPARSE": "1"}),
        _case("sparse_auto", env={"WIN_SPARSE": "auto"}),
        _case("sparse1_h128", env={"WIN_SPARSE": "1"}, hidden_sizes=(128, 50)),
        _case("h512", hidden_sizes=(512,)),
        _case("three_layers", hidden_sizes=(64, 32, 48)),
        _case("k64", n_components=64),
        _case("k65", n_components=65),
        _case("fixed_priors", learn_priors=False),
        _case("sgd", solver="sgd"),
        # NeuralLDA
        _case("lda", model_type="LDA"),
        _case("lda_b256", model_type="LDA", batch_size=256),
        # the large-batch plan
        _case("lb256", batch_size=256),
        _case("lb256_k208", batch_size=256, n_components=208),
        _case("lb256_k209", batch_size=256, n_components=209),
        _case("lb512", batch_size=512),
        _case("lb_b32_k300", batch_size=32, n_components=300),
        _case("lb256_sgd", batch_size=256, solver="sgd"),
        _case("lb256_gemm", env={"LB_GEMM": "1"}, batch_size=256),
        _case("lb256_gemm0", env={"LB_GEMM": "0"}, batch_size=256),
        _case("lb256_v112k", batch_size=256, input_size=112000),
        _case("lb256_sparse1", env={"WIN_SPARSE": "1"}, batch_size=256),
        _case("lb256_v112k_dense", env={"WIN_SPARSE": "0"}, batch_size=256, input_size=112000),
        _case("lb512_k512", batch_size=512, n_components=512, hidden_sizes=(64, 64)),
        # over the LDS budget (NeuralLDA's beta backward at K = 256 rows of 256)
        _case("lda_b256_k256_over_budget", model_type="LDA", batch_size=256, n_components=256),
        # CombinedTM, C = 96
        *[_case("ctm" + "".join("_%s%s" % (k.lower(), v) for k, v in env.items()), "combined",
                env=env, input_size=3000, n_components=20, contextual_size=96)
          for env in ({}, {"CTX_FULL": "1"}, {"CTX_FULL": "1", "CTX_RS": "0"}, {"CTX_RS": "1"},
                      {"CTX_BWDPP": "1"}, {"CTX_FULL": "0"}, {"CTX_BWDPP": "0"},
                      {"CTX_FULL": "auto", "CTX_BWDPP": "auto"}, {"WIN_SPARSE": "1"})],
        _case("ctm_v74k", "combined", input_size=74000, n_components=20, contextual_size=96),
        _case("ctm_v74k_full0_pp0", "combined", env={"CTX_FULL": "0", "CTX_BWDPP": "0"},
              input_size=74000, n_components=20, contextual_size=96),
        _case("ctm_v74k_rs0", "combined", env={"CTX_RS": "0"},
              input_size=74000, n_components=20, contextual_size=96),
        _case("ctm_bf16", "combined", input_size=3000, n_components=20, contextual_size=96,
              matmul_dtype="bf16"),
        _case("ctm_c98_host_gemms", "combined", input_size=3000, n_components=20, contextual_size=98),
        _case("ctm_labels", "combined", input_size=3000, n_components=20, contextual_size=96,
              label_size=5),
        _case("ctm_b128", "combined", input_size=3000, n_components=20, contextual_size=96,
              batch_size=128),
        _case("ctm_h512_lds_fallback", "combined", input_size=3000, n_components=20,
              contextual_size=96, hidden_sizes=(512, 50)),
        # over the LDS budget (win_update's dense tile at H0 = 256, 128 rows)
        _case("ctm_b128_h256_over_budget", "combined", input_size=3000, n_components=20,
              contextual_size=96, batch_size=128, hidden_sizes=(256, 50)),
        # ZeroShotTM
        _case("zeroshot", "zeroshot", contextual_size=768),
        _case("zeroshot_labels", "zeroshot", contextual_size=768, label_size=5),
        # batched launches
        *[_case("batched_headline_m%d" % M, M=M) for M in (1, 2, 8, 17)],
        _case("batched_v200_m2", M=2, input_size=200),
        _case("batched_v6100_m8", M=8, input_size=6100),      # 96 tiles: the 8-wave window's edge
        _case("batched_v6200_m8", M=8, input_size=6200),      # 97
        _case("batched_v1500_m8", M=8, input_size=1500),      # 24 tiles: 6 waves per SIMD by default
        _case("batched_k65_m8", M=8, n_components=65),
        _case("batched_k200_m8", M=8, input_size=3000, n_components=200),
        _case("batched_bf16_m8", M=8, matmul_dtype="bf16"),
        _case("batched_lda_m8", M=8, model_type="LDA"),
        _case("batched_lda_m8_keep", M=8, env={"BATCH_STRIP": "keep"}, model_type="LDA"),
        _case("batched_ctm_v5000_m8", "combined", M=8, input_size=5000, n_components=20,
              contextual_size=96),
        _case("batched_ctm_v5000_m8_own", "combined", M=8, env={"CTX_FULL": "0", "CTX_BWDPP": "0"},
              input_size=5000, n_components=20, contextual_size=96),
        _case("batched_zeroshot_m2", "zeroshot", M=2, contextual_size=768),
        *[_case("batched_post_rows_%s_m%d" % (v, M), M=M, env={"POST_ROWS": v})
          for v in ("auto", "serial2", "2", "4") for M in (2, 8)],
        _case("batched_post_rows_bad", M=2, env={"POST_ROWS": "3"}),
        _case("batched_post_rows_bad_m1", M=1, env={"POST_ROWS": "3"}),
        _case("batched_post_rows_4_k200", M=2, env={"POST_ROWS": "4"}, input_size=3000,
              n_components=200),
        # the joint rows' vectors do not fit the LDS
        _case("batched_post_rows_4_k128_no_fit", M=2, env={"POST_ROWS": "4"}, input_size=3000,
              n_components=128, hidden_sizes=(256, 256)),
        *[_case("batched_bwd_waves_%s_m%d" % (v, M), M=M, env={"BWD_WAVES": v})
          for v in ("auto", "16", "8") for M in (2, 8)],
        _case("batched_bwd_waves_8_k65", M=2, env={"BWD_WAVES": "8"}, n_components=65),
        _case("batched_bwd_waves_bad", M=2, env={"BWD_WAVES": "4"}),
        *[_case("batched_win_waves_%s_m%d" % (v, M), M=M, env={"WIN_WAVES": v})
          for v in ("auto", "8", "6") for M in (2, 8)],
        _case("batched_win_waves_6_h128", M=2, env={"WIN_WAVES": "6"}, hidden_sizes=(128, 50)),
        _case("batched_win_waves_bad", M=2, env={"WIN_WAVES": "7"}),
        _case("batched_keep_m8", M=8, env={"BATCH_STRIP": "keep"}),
        _case("batched_fill_m8", M=8, env={"BATCH_STRIP": "fill"}),
        _case("batched_postfold0_m8", M=8, env={"POSTFOLD": "0"}),
        _case("batched_postfold1_m8", M=8, env={"POSTFOLD": "1"}),
        _case("batched_postfold_auto_m8", M=8, env={"POSTFOLD": "auto"}),
        _case("batched_sparse1_m8", M=8, env={"WIN_SPARSE": "1"}),
    ]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), "duplicate case names"
    return out


CASES = _cases()


def value_fields(m) -> dict:
    """Every value field of a GfkModel: no pointers, no arrays of pointers, no seed, none of
    ADDRESS_FIELDS."""
    from gfedntm_amd.ops import kernel_abi as abi
    out = {}
    for name, typ in abi.GfkModel._fields_:
        if typ is abi.P or name == "seed" or name in ADDRESS_FIELDS:
            continue
        if isinstance(typ, type) and issubclass(typ, C.Array):
            if typ._type_ is abi.P:
                continue
            out[name] = list(getattr(m, name))
        else:
            out[name] = getattr(m, name)
    return out


class knob_env:
    """The case's GFEDNTM_* plan knobs set, every other plan knob unset, for the block."""

    def __init__(self, env):
        self.env = {"GFEDNTM_" + k: v for k, v in env.items()}

    def __enter__(self):
        self.saved = {k: os.environ.pop(k, None) for k in ("GFEDNTM_" + k for k in KNOBS)}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def build_models(case, device="cuda"):
    """The case's max(M, 1) models on ``device`` (fused backend)."""
    import torch
    from gfedntm_amd.models import AVITM, CombinedTM, ZeroShotTM
    cls = {"avitm": AVITM, "combined": CombinedTM, "zeroshot": ZeroShotTM}[case["model"]]
    kw = dict(case["kw"])
    kw["hidden_sizes"] = tuple(kw["hidden_sizes"])
    torch.manual_seed(0)
    return [cls(verbose=False, backend="fused", device=device, num_epochs=1, **kw)
            for _ in range(max(case["M"], 1))]


def record(case, device="cuda") -> dict:
    """Construct the case on the device and read its plan back (see the module docstring)."""
    import logging
    import torch
    from gfedntm_amd.ops.engine import BatchedSteps
    rec = {"name": case["name"], "model": case["model"], "M": case["M"], "env": case["env"],
           "kw": {k: list(v) if isinstance(v, tuple) else v for k, v in case["kw"].items()},
           "cu": torch.cuda.get_device_properties(device).multi_processor_count}
    logging.getLogger("gfedntm_amd.engine").setLevel(logging.ERROR)
    tms = None
    with knob_env(case["env"]):
        try:
            tms = build_models(case, device)
            e = tms[0].engine
            slot = e.flat.slots.get("inf_net.adapt_bert.weight")
            rec.update(ldb=int(e._m.ldb), n_total=int(e.flat.n_total),
                       aligned=None if slot is None else slot.offset % 4 == 0,
                       n_w=int(e._u.n_w), n_v=int(e._u.n_v),
                       m=value_fields(e._m), update_mode=int(e.update_mode),
                       launch_plan=e.launch_plan, gemm_dtypes=e.gemm_dtypes,
                       ctx_fallback_reason=e.ctx_fallback_reason, phases=list(e.phases()))
            if case["M"]:
                bs = BatchedSteps([tm.engine for tm in tms])
                bs.prepare()
                rec.update(host=value_fields(bs._host), batched_phases=list(bs._phases),
                           batched_plan=bs.plan)
        except Exception as ex:          # noqa: BLE001 (the record is the exception)
            rec["error"] = [type(ex).__name__, str(ex)]
    del tms
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def main(argv):
    out = argv[1] if len(argv) > 1 else GOLDEN
    recs = []
    for case in CASES:
        recs.append(record(case))
        print(case["name"], recs[-1].get("error", "ok"), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in recs) + "\n]\n")
    print("wrote %d cases to %s" % (len(recs), out))


if __name__ == "__main__":
    main(sys.argv)
