"""GFEDNTM_WIN_WAVES -> stage bits 9 / 24 of the batched win_update (no device needed)."""
import os
import re

import pytest

from gfedntm_amd.ops import engine
from gfedntm_amd.ops import kernel_abi as abi

BIT = abi.WIN_WAVES6
B8 = engine.STAGE_WIN_BATCH8
CUS = 256
# a launch like the headline's: 74 tiles plus the job workgroups per client (n_wg = 91 below),
# hidden (50, 50), the 8-wave dense tiles (8 x (74 + 8) > 2 x 256), 37 KB of LDS
HEAD = dict(dense=True, batch8=True, fused=True, H0=50, lds_bytes=37 * 1024)


def _flag(M, n_wg, knob="auto", **kw):
    return engine.win_waves_flag(M, n_wg, CUS, **{**HEAD, **kw}, knob=knob)


def test_bit_mirrors_the_kernel_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "csrc", "gfk_common.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int GFK_WIN_WAVES6 = (\d+);", src).group(1)) == BIT == 1 << 24
    assert engine.STAGE_WIN_WAVES6 == BIT
    with open(os.path.join(root, "csrc", "update.hip")) as f:
        assert int(re.search(r"constexpr int WIN_BATCH8 = (\d+);", f.read()).group(1)) == B8 == 1 << 9
    others = [v for k, v in vars(engine).items()
              if k.startswith("STAGE_") and k not in ("STAGE_WIN_WAVES6", "STAGE_PLANS")]
    assert all(not v & BIT for v in others)


def test_lds_budget_is_a_third_of_a_cu():
    assert engine.WIN6_LDS == 160 * 1024 // 3 == 54613


def test_auto_takes_launches_that_three_workgroups_per_cu_hold_at_once():
    # 8 clients: 8 n_wg <= 3 x 256  <=>  n_wg <= 96
    assert _flag(8, 91) == BIT            # the headline
    assert _flag(8, 96) == BIT
    assert _flag(8, 97) == 0
    # 2 clients: n_wg <= 384
    assert _flag(2, 384) == BIT
    assert _flag(2, 385) == 0
    # 3 clients (plain placement): n_wg <= 256
    assert _flag(3, 256) == BIT
    assert _flag(3, 257) == 0


def test_auto_never_adds_the_eight_wave_shape_itself():
    # the launch keeps its 16-wave tiles: no 6-waves-per-SIMD instance of those
    assert _flag(8, 20, batch8=False) == 0
    assert _flag(2, 12, batch8=False) == 0


def test_one_client_never_takes_it():
    for knob in ("auto", "8", "6"):
        assert _flag(1, 91, knob) == 0
        assert _flag(1, 91, knob, H0=100) == 0      # (not a batched launch: no error either)


@pytest.mark.parametrize("kw", [dict(dense=False), dict(fused=False), dict(H0=65),
                                dict(lds_bytes=engine.WIN6_LDS + 1)])
def test_no_instance(kw):
    assert _flag(8, 91, **kw) == 0
    assert _flag(2, 12, **kw) == 0
    with pytest.raises(RuntimeError, match="GFEDNTM_WIN_WAVES=6"):
        _flag(8, 91, "6", **kw)
    with pytest.raises(RuntimeError, match="GFEDNTM_WIN_WAVES=6"):
        _flag(2, 12, "6", batch8=False, **kw)
    # 8 forces the shape wherever the dense tiles run, whatever the other limits
    assert _flag(8, 91, "8", **kw) == (B8 if kw.get("dense", True) else 0)


def test_instance_limits():
    assert _flag(8, 91, H0=64) == BIT
    assert _flag(8, 91, H0=1) == BIT
    assert _flag(8, 91, lds_bytes=engine.WIN6_LDS) == BIT


def test_knob_forces_either_budget_on_every_batched_launch():
    for M, n_wg, b8 in ((2, 12, False), (3, 12, False), (8, 91, True), (8, 97, True), (2, 1000, True)):
        assert _flag(M, n_wg, "6", batch8=b8) == B8 | BIT
        assert _flag(M, n_wg, "8", batch8=b8) == B8
    with pytest.raises(ValueError):
        _flag(8, 91, "4")
    with pytest.raises(ValueError):
        _flag(8, 91, "16")
    with pytest.raises(ValueError):
        _flag(1, 91, "")
