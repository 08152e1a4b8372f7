"""CPU: every kernel of the connected-components unit (vpt_volume_components.hip) compiles for gfx950 without scratch memory or register
spills, with at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_rank_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_components_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_components"])
    # k_label_tiles<T, CONN>: T in {uint8_t (h), uint16_t (t)}, CONN in {6, 18, 26}
    tiles = {k: v for k, v in usage.items() if re.match(r"_Z13k_label_tilesI[ht]Li(6|18|26)EE", k)}
    assert len(tiles) == 6, sorted(usage)
    # k_merge<CONN>
    merge = {k: v for k, v in usage.items() if re.match(r"_Z7k_mergeILi(6|18|26)EE", k)}
    assert len(merge) == 3, sorted(usage)
    # the label emitter: k_pair<T, RankChannel> (vpt_volume_field.h), instantiated here
    emit = {k: v for k, v in usage.items() if re.match(r"_Z6k_pairI[ht]11RankChannelE", k)}
    assert len(emit) == 2, sorted(usage)
    # flatten, sizes, census, compaction, the rank table, the rank write
    plain = {k: v for k, v in usage.items() if re.match(r"_Z\d+k_(flatten|sizes|census|compact|rank_table|ranks)P", k)}
    assert len(plain) == 6, sorted(usage)
    assert len(usage) == 17, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    for name, u in tiles.items():                                # the tile's labels are staged in LDS
        assert u.get("LDS Size", 0) >= 66 * 10 * 6 * 2, (name, u)
