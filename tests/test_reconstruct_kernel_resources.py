"""CPU: every kernel of the reconstruction unit (vpt_volume_reconstruct.hip) compiles for gfx950 without scratch memory or register spills
and with an occupancy of at least 2, and the tile kernel's LDS is the two staged arrays and its flags: the conditions of the sibling
units (tests/test_components_kernel_resources.py).  The instantiations are listed, so none the contract does not admit is compiled and none
escapes the conditions.  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage

BYTES = {'h': 1, 't': 2}                                          # uint8_t, uint16_t
PADDED = 66 * 10 * 6                                              # the 64 x 8 x 4 tile with its one-voxel rim
# the directions word (4 bytes), the 64 words the device library's workgroup OR (__syncthreads_or) reduces the waves' votes through, and up to
# 16 bytes of alignment between the four objects
FLAG_BYTES = 4 + 64 * 4 + 16


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_reconstruct_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_reconstruct"])
    # k_recon_tiles<T, CONN>: T in {uint8_t (h), uint16_t (t)}, CONN in {6, 18, 26}
    tiles = {m.groups(): name for name in usage for m in [re.match(r"_Z13k_recon_tilesI([ht])Li(\d+)EE", name)] if m}
    assert set(tiles) == {(t, c) for t in BYTES for c in ('6', '18', '26')}, sorted(usage)
    # k_recon_seed<T>, k_recon_finish<T>
    seed = {m.group(1): name for name in usage for m in [re.match(r"_Z12k_recon_seedI([ht])E", name)] if m}
    finish = {m.group(1): name for name in usage for m in [re.match(r"_Z14k_recon_finishI([ht])E", name)] if m}
    assert set(seed) == set(BYTES) and set(finish) == set(BYTES), sorted(usage)
    assert len(usage) == 10, sorted(usage)                        # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    for (t, _), name in tiles.items():                            # r and the mask, each with its rim, and the flags
        lds = usage[name].get("LDS Size", 0)
        assert PADDED * 2 * BYTES[t] <= lds <= PADDED * 2 * BYTES[t] + FLAG_BYTES, (name, usage[name])
    for name in list(seed.values()) + list(finish.values()):      # the streaming kernels use none
        assert usage[name].get("LDS Size", 0) == 0, (name, usage[name])
