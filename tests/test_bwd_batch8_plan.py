"""GFEDNTM_BWD_WAVES -> stage bit 23 of the batched ProdLDA tile backward (no device needed)."""
import os
import re

import pytest

from gfedntm_amd.ops import engine
from gfedntm_amd.ops import kernel_abi as abi

BIT = abi.BWD_BATCH8
CUS = 256
# the headline: K = 50 (theta_d stride 50), 64 rows
HEAD = dict(bmax=64, K=50, bf16=False, kq=1, bwd_pre=0, lds_bytes=engine.bwd8_lds_bytes(64, 50, 50))


def _flag(M, n_tiles, knob="auto", **kw):
    return engine.bwd_batch8_flag(M, n_tiles, CUS, **{**HEAD, **kw}, knob=knob)


def test_bit_mirrors_the_kernel_header():
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "gfk_common.h")
    with open(hdr) as f:
        src = f.read()
    assert int(re.search(r"constexpr int GFK_BWD_BATCH8 = (\d+);", src).group(1)) == BIT == 1 << 23
    assert engine.STAGE_BWD_BATCH8 == BIT
    # no other stage bit of the engine shares it
    others = [v for k, v in vars(engine).items() if k.startswith("STAGE_") and k not in ("STAGE_BWD_BATCH8", "STAGE_PLANS")]
    assert all(not v & BIT for v in others)


def test_lds_budget_is_a_third_of_a_cu():
    assert engine.BWD8_LDS == 160 * 1024 // 3 == 54613
    # theta_d 64 x 50, the logit-tile / beta-block region 64 x 66, dt 64 x 66, lse + S + rstd
    assert engine.bwd8_lds_bytes(64, 50, 50) == 4 * (3200 + 4224 + 4224 + 192) == 47360
    assert engine.bwd8_lds_bytes(64, 16, 18) == 4 * (64 * 18 + 4096 + 4224 + 192)    # one k tile: the logit tile is larger
    assert engine.bwd8_lds_bytes(64, 64, 66) <= engine.BWD8_LDS


def test_auto_takes_the_window_between_two_and_three_per_cu():
    # 8 clients: 2 x 256 < 8 n_tiles <= 3 x 256  <=>  65 <= n_tiles <= 96
    assert _flag(8, 64) == 0          # 512 tiles: two 16-wave workgroups per CU hold them
    assert _flag(8, 65) == BIT
    assert _flag(8, 74) == BIT        # the headline, V = 4718
    assert _flag(8, 96) == BIT        # 768 = 3 CUs
    assert _flag(8, 97) == 0
    # 2 clients: 257 <= n_tiles <= 384
    assert _flag(2, 256) == 0
    assert _flag(2, 257) == BIT
    assert _flag(2, 384) == BIT
    assert _flag(2, 385) == 0
    assert _flag(2, 4) == 0


def test_one_client_never_takes_it():
    for knob in ("auto", "16", "8"):
        assert _flag(1, 74, knob) == 0
        assert _flag(1, 600, knob) == 0
        assert _flag(1, 74, knob, K=65) == 0      # (not a batched launch: no error either)


@pytest.mark.parametrize("kw", [dict(K=65), dict(bmax=32), dict(bf16=True), dict(bwd_pre=2), dict(kq=4),
                                dict(kq=0), dict(lds_bytes=engine.BWD8_LDS + 1)])
def test_no_instance(kw):
    assert _flag(8, 74, **kw) == 0
    assert _flag(2, 300, **kw) == 0
    assert _flag(8, 74, "16", **kw) == 0
    with pytest.raises(RuntimeError):
        _flag(8, 74, "8", **kw)
    with pytest.raises(RuntimeError):
        _flag(2, 4, "8", **kw)


def test_instance_limits():
    assert _flag(8, 74, K=64, lds_bytes=engine.bwd8_lds_bytes(64, 64, 66)) == BIT
    assert _flag(8, 74, lds_bytes=engine.BWD8_LDS) == BIT
    assert _flag(8, 74, bmax=64) == BIT


def test_knob_forces_either_shape_on_every_batched_launch():
    for M, n_tiles in ((2, 1), (2, 4), (8, 64), (8, 74), (8, 97), (2, 1000)):
        assert _flag(M, n_tiles, "8") == BIT
        assert _flag(M, n_tiles, "16") == 0
    with pytest.raises(ValueError):
        _flag(8, 74, "4")
    with pytest.raises(ValueError):
        _flag(1, 74, "")


def test_bwd_kq_mirrors_the_launcher():
    # 4 k ranges only where the tiles outnumber the workgroups and K has 4 k tiles
    assert engine.bwd_kq(74, 74, 50) == 1
    assert engine.bwd_kq(1750, 256, 50) == 4
    assert engine.bwd_kq(1750, 256, 48) == 1
    assert engine.bwd_kq(1750, 1750, 200) == 1
