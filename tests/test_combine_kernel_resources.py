"""CPU: every kernel of the combining unit (vpt_volume_combine.hip) compiles for gfx950 without scratch memory, register spills or LDS and
with an occupancy of at least 2: the conditions of the sibling units (tests/test_resample_kernel_resources.py).  The instantiations are
listed, so none the contract does not admit is compiled and none escapes the conditions.  These are conditions, not measurements (DESIGN.md
records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage

TYPES = {'h': 'uint8_t', 't': 'uint16_t'}
MASK, PAIR = 0, 5


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_combine_kernels_use_no_scratch_no_lds_and_share_a_cu():
    usage = resource_usage(["vpt_volume_combine"])
    # k_combine<TA, TB, STRIDE_B, OP>: TA, TB in {uint8_t (h), uint16_t (t)}, b of one or two channels
    combine = {}
    for name in usage:
        m = re.match(r"_Z9k_combineI([ht])([ht])Li([12])ELi(\d)EE", name)
        if m:
            combine[(m.group(1), m.group(2), int(m.group(3)), int(m.group(4)))] = name
    # MASK reads a b of either width; every other op has b's channel as wide as a
    admitted = {(ta, tb, stride, MASK) for ta in TYPES for tb in TYPES for stride in (1, 2)}
    admitted |= {(t, t, stride, op) for t in TYPES for stride in (1, 2) for op in range(MASK + 1, PAIR + 1)}
    assert len(admitted) == 28 and set(combine) == admitted, sorted(set(combine) ^ admitted)
    # k_compare<TA, TB, STRIDE_B>: mixed widths are taken
    compare = {m.groups(): name for name in usage for m in [re.match(r"_Z9k_compareI([ht])([ht])Li([12])EE", name)] if m}
    assert set(compare) == {(ta, tb, stride) for ta in TYPES for tb in TYPES for stride in '12'}, sorted(compare)
    assert len(usage) == 36, sorted(usage)                        # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) == 0, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
