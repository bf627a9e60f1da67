"""The launch plans recorded in tests/golden/step_plans.json (tools/dump_plans.py, on an MI355X
with the engine as it was before the planner moved into gfedntm_amd/ops/plan.py), replayed.

Without a GPU: each case's recorded inputs -- the constructor arguments, the knobs, the CU
count, beta's row stride, the flat buffer's length and alignment fact, the job counts, the
update mode -- go through ops/plan.py alone, and every plan field of the descriptor, phase
list, plan string, GEMM type and error comes out as recorded.  (The update mode is the engine's
decision, not the planner's; its rule is asserted next to it.)  On a GPU with the recorded CU
count: the engines themselves, every value field of ``_m`` and ``_host``.  No step runs.
"""
import json
import os
import re
from types import SimpleNamespace

import pytest

from gfedntm_amd.ops import kernel_abi as abi
from gfedntm_amd.ops import native, plan

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "step_plans.json")
with open(GOLDEN) as f:
    RECS = json.load(f)
IDS = [r["name"] for r in RECS]

# what fill_shape and the two planners set (the other value fields are the engine's: rates,
# optimizer constants, data-bound sizes)
PLAN_FIELDS = ("bmax", "V", "K", "n_hidden", "H", "act", "kind", "input", "C", "L", "vb", "n_tiles",
               "dec_grid", "learn_priors", "stage_flags", "kt", "n_dpart", "lb_fused", "ctx_fused",
               "ctx_kb", "ctx_ckb", "mm_bf16", "ctx_parts", "lab_on", "lab_off", "bwd_pre", "ldb",
               "ctx_bgrid")
# errors of FusedEngine's construction that are not the planner's
SUPPORTS_LDS = re.compile(r"fused engine unsupported: LDS budget exceeded \((\d+) B\)")

needs_lib = pytest.mark.skipif(not native.kernels_available(), reason="kernel library not built")


def _tm(rec):
    kw = dict(model_type="prodLDA", activation="softplus", matmul_dtype="fp32", learn_priors=True,
              solver="adam", label_size=0, contextual_size=0)
    kw.update(rec["kw"])
    kw.update(kind="avitm" if rec["model"] == "avitm" else "ctm", inference_type=rec["model"])
    return SimpleNamespace(**kw)


def _knobs(rec):
    return plan.Knobs.from_env({"GFEDNTM_" + k: v for k, v in rec["env"].items()})


def _fields(m, names):
    return {k: list(getattr(m, k)) if k == "H" else getattr(m, k) for k in names}


def _plan_one(rec, lib):
    tm = _tm(rec)
    m = plan.fill_shape(abi.GfkModel(), tm, plan.engine_bmax(tm), rec.get("ldb"))
    sp = plan.plan_step(lib, m, rec["cu"], _knobs(rec), tm.solver, rec.get("n_total", 0),
                        rec.get("aligned") is not False)
    return tm, m, sp


@needs_lib
@pytest.mark.parametrize("rec", RECS, ids=IDS)
def test_planner_reproduces_the_recorded_plan(rec):
    lib = native.kernels()
    err = rec.get("error")
    if err and "m" not in rec:
        # the engine was never built: supports() refused the shape for its LDS; the one LDS
        # search gives the recorded need, and the planner on its own refuses the shape too
        need = SUPPORTS_LDS.fullmatch(err[1])
        assert err[0] == "RuntimeError" and need, err
        tm = _tm(rec)
        assert plan.lds_required(lib, tm, plan.engine_bmax(tm)) == int(need.group(1))
        with pytest.raises(RuntimeError, match=r"needs %s B of LDS \(> %d\)" % (need.group(1), plan.LDS_LIMIT)):
            _plan_one(rec, lib)
        return
    tm, m, sp = _plan_one(rec, lib)
    assert _fields(m, PLAN_FIELDS) == {k: rec["m"][k] for k in PLAN_FIELDS}
    assert sp.ctx_fallback == rec["ctx_fallback_reason"]
    assert plan.lds_required(lib, tm, m.bmax) <= plan.LDS_LIMIT          # supports() said yes
    # the engine's rule for the update mode
    mode = rec["update_mode"]
    assert mode == (plan.UPDATE_FUSED if tm.solver == "adam" and not m.stage_flags & plan.STAGE_LB
                    and sp.ctx_fallback is None else plan.UPDATE_GRAD)
    assert rec["m"]["update_mode"] == mode
    assert rec["m"]["lab_in_enc"] == int(bool(m.lab_on and m.ctx_fused))
    assert plan.step_phases(m, mode) == rec["phases"]
    assert plan.launch_plan(m, mode) == rec["launch_plan"]
    assert plan.gemm_dtypes(m) == rec["gemm_dtypes"]
    if not rec["M"]:
        assert err is None
        return
    args = (lib, m, rec["M"], rec["cu"], _knobs(rec), rec["n_w"], rec["n_v"], mode, sp.postfold_ok,
            rec["phases"])
    if err:
        with pytest.raises({"RuntimeError": RuntimeError, "ValueError": ValueError}[err[0]],
                           match="^" + re.escape(err[1]) + "$"):
            plan.plan_batched(*args)
        return
    before = bytes(m)
    bp = plan.plan_batched(*args)
    assert bytes(m) == before                       # the client's own descriptor is not touched
    host = dict(rec["m"], n_batch=rec["M"], stage_flags=bp.stage_flags, dec_grid=bp.dec_grid,
                ctx_bgrid=bp.ctx_bgrid)
    assert host == rec["host"]
    assert bp.phases == rec["batched_phases"] and bp.text == rec["batched_plan"]
    # gfk_setup exactly where the launch runs a kernel shape the engines' plans did not
    new = bp.stage_flags & ~m.stage_flags & (plan.STAGE_POST_JOINT | plan.STAGE_CTX_FULL | plan.STAGE_CTX_BWDPP)
    assert (bp.setup_flags is not None) == bool(new)
    if new:
        assert bp.setup_flags & new == new and not bp.setup_flags & ~bp.stage_flags


@needs_lib
def test_planner_lds_errors_not_reachable_through_supports():
    """supports() refuses every shape found so far that the planner's own LDS checks refuse
    (the over-budget cases of the file), so those two errors are reached here directly."""
    lib = native.kernels()
    over = {r["name"]: r for r in RECS if r["name"].endswith("over_budget")}
    with pytest.raises(RuntimeError, match=r"^large-batch plan needs 168448 B of LDS \(> 163840\)$"):
        _plan_one(over["lda_b256_k256_over_budget"], lib)
    with pytest.raises(RuntimeError, match=r"^fused step needs 172544 B of LDS \(> 163840\)$"):
        _plan_one(over["ctm_b128_h256_over_budget"], lib)


@needs_lib
def test_auto_post_rows_fall_back_to_serial_rows_where_joint_rows_do_not_fit():
    """Not in the file: the joint rows add 3 to 7 KB to post_bwd's LDS, and at the shapes where
    that crosses the limit (the engine's own need above 157 KB) gfk_setup refuses the engine's
    own plan on the device -- K = 64, hidden (192, 64), 161344 B of dynamic LDS next to the
    kernels' static arrays -- so the engine cannot be recorded.  The planner alone:"""
    lib = native.kernels()
    rec = {"model": "avitm", "env": {}, "cu": 256,
           "kw": dict(input_size=3000, n_components=64, hidden_sizes=[192, 64], batch_size=64)}
    tm, m, sp = _plan_one(rec, lib)
    ph = plan.step_phases(m, plan.UPDATE_FUSED)
    bp = plan.plan_batched(lib, m, 8, 256, plan.Knobs(), 5, 6, plan.UPDATE_FUSED, sp.postfold_ok, ph)
    assert bp.stage_flags >> 20 & 7 == 1 and bp.setup_flags is None
    with pytest.raises(RuntimeError, match="GFEDNTM_POST_ROWS=2: the rows' vectors do not fit the LDS"):
        plan.plan_batched(lib, m, 8, 256, plan.Knobs(post_rows="2"), 5, 6, plan.UPDATE_FUSED, sp.postfold_ok, ph)


def test_the_table_leaves_no_branch_out():
    flags = [r[k]["stage_flags"] for r in RECS for k in ("m", "host") if k in r]
    for bit in (0, 1, 2, 4, 5, 9, 12, 15, 16, 19, 20, 21, 22, 23, 24):      # docs/DESIGN.md's table
        assert any(f >> bit & 1 for f in flags), f"bit {bit} is set in no case"
        assert any(not f >> bit & 1 for f in flags), f"bit {bit} is clear in no case"
    values = {"FWD_STRIP": "auto 1 0", "POSTFOLD": "auto 1 0", "BWD_PRE": "3 2 0", "CTX_FULL": "auto 1 0",
              "CTX_RS": "1 0", "CTX_BWDPP": "auto 1 0", "WIN_SPARSE": "auto 1 0", "LB_GEMM": "0 1",
              "BATCH_STRIP": "fill keep", "POST_ROWS": "auto serial2 2 4", "BWD_WAVES": "auto 16 8",
              "WIN_WAVES": "auto 8 6"}
    assert sorted(values) == sorted(f.name.upper() for f in plan.Knobs.__dataclass_fields__.values())
    for knob, vals in values.items():
        seen = {r["env"][knob] for r in RECS if knob in r["env"]}
        assert set(vals.split()) <= seen, f"GFEDNTM_{knob}: no case at {set(vals.split()) - seen}"
    errors = [r["error"][1] for r in RECS if "error" in r]
    for msg in ("GFEDNTM_POST_ROWS='3': expected", "the rows' vectors do not fit the LDS",
                "GFEDNTM_BWD_WAVES=8: no 8-wave", "GFEDNTM_BWD_WAVES='4': expected",
                "GFEDNTM_WIN_WAVES=6: no 6-waves", "GFEDNTM_WIN_WAVES='7': expected",
                "LDS budget exceeded"):             # (the planner's two: the test above)
        assert any(msg in e for e in errors), msg
    # the shapes the conditions' edges were chosen for, at the recorded CU count
    by = {r["name"]: r for r in RECS}
    cu = by["headline"]["cu"]
    big, pre2, pre0 = (by[n]["m"] for n in ("v112k_k200", "v112k_k200_pre2", "v112k_k200_pre0"))
    assert big["n_tiles"] == 1750 and big["n_dpart"] in (cu // 2, cu // 4) and big["bwd_pre"] == 3
    assert (pre2["bwd_pre"], pre0["bwd_pre"]) == (2, 0)
    assert by["v112k_k48"]["m"]["n_dpart"] == cu
    ks = by["v130_k256_ksplit"]["m"]
    assert ks["n_dpart"] == ks["n_tiles"] - 1 == 2
    assert (by["v8191"]["m"]["ldb"], by["v8192"]["m"]["ldb"]) == (8191, 8192) and by["v33k_two_per_cu"]["m"]["ldb"] == 33024
    assert by["ctm_c98_host_gemms"]["ctx_fallback_reason"] and by["ctm_h512_lds_fallback"]["ctx_fallback_reason"]
    assert not by["batched_post_rows_bad_m1"].get("error")      # one client never raises


@pytest.mark.gpu
def test_engines_take_the_recorded_plans():
    import torch
    from tools import dump_plans
    cu = torch.cuda.get_device_properties("cuda").multi_processor_count
    if cu != RECS[0]["cu"]:
        pytest.skip(f"recorded on {RECS[0]['cu']} CUs, this device has {cu}")
    assert [c["name"] for c in dump_plans.CASES] == IDS
    for case, rec in zip(dump_plans.CASES, RECS):
        assert dump_plans.record(case) == rec, case["name"]
