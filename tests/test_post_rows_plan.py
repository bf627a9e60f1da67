"""GFEDNTM_POST_ROWS -> stage bits of the batched post_bwd (no device needed)."""
import pytest

from gfedntm_amd.ops import engine
from gfedntm_amd.ops import kernel_abi as abi

R2, JOINT, R4 = abi.POST_ROWS2, abi.POST_JOINT, abi.POST_ROWS4


def test_bits_mirror_the_kernel_header():
    import os
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "gfk_common.h")
    with open(hdr) as f:
        src = f.read()
    for name, bit in (("GFK_POST_ROWS2", R2), ("GFK_POST_JOINT", JOINT), ("GFK_POST_ROWS4", R4)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) == bit
    assert (R2, JOINT, R4) == (1 << 20, 1 << 21, 1 << 22)
    assert (engine.STAGE_POST_ROWS2, engine.STAGE_POST_JOINT, engine.STAGE_POST_ROWS4) == (R2, JOINT, R4)


def test_forced_shapes_apply_to_every_batched_launch():
    want = {"serial2": R2, "2": R2 | JOINT, "4": R2 | JOINT | R4}
    for knob, bits in want.items():
        # also where M (bmax + 1) one-row workgroups would fit one round of the CUs
        assert engine.post_rows_flags(2, 16, 256, knob) == bits
        assert engine.post_rows_flags(8, 64, 256, knob) == bits
        assert engine.post_rows_flags(1, 64, 256, knob) == 0      # one client: the one-row shape
    with pytest.raises(ValueError):
        engine.post_rows_flags(2, 16, 256, "3")


def test_auto_keeps_the_condition_of_bit_20():
    auto = abi.POST_ROWS_SHAPES[engine.POST_ROWS_AUTO]
    assert auto & R2
    assert engine.post_rows_flags(8, 64, 256, "auto") == auto      # 8 x 65 workgroups > 256 CUs
    assert engine.post_rows_flags(3, 64, 256, "auto") == 0         # 3 x 65 fit one round
    assert engine.post_rows_flags(1, 512, 256, "auto") == 0
