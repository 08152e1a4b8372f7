"""CPU: every kernel of the watershed unit (vpt_volume_watershed.hip) compiles for gfx950 without scratch memory or register spills, with at
most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_components_kernel_resources.py).  These are conditions, not measurements (DESIGN.md "Watershed" records the figures the
compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_watershed_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_watershed"])
    # k_ws_classify, k_ws_plateau, k_ws_links, k_ws_merge <T, CONN>: T in {uint8_t (h), uint16_t (t)}, CONN in {6, 18, 26}
    tiled = {}
    for kernel in ("k_ws_classify", "k_ws_plateau", "k_ws_links", "k_ws_merge"):
        found = {k: v for k, v in usage.items() if re.match(r"_Z%d%sI[ht]Li(6|18|26)EE" % (len(kernel), kernel), k)}
        assert len(found) == 6, (kernel, sorted(usage))
        tiled[kernel] = found
    # the snapshot of one channel of a two-channel relief: k_ws_channel<T>
    channel = {k: v for k, v in usage.items() if re.match(r"_Z12k_ws_channelI[ht]E", k)}
    assert len(channel) == 2, sorted(usage)
    assert len(usage) == 26, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    pad = 66 * 10 * 6
    for name, u in tiled["k_ws_classify"].items():               # the keys of the tile and its rim
        assert u.get("LDS Size", 0) >= pad * 4, (name, u)
    for name, u in tiled["k_ws_plateau"].items():                # keys and d
        assert u.get("LDS Size", 0) >= pad * 8, (name, u)
    for name, u in tiled["k_ws_links"].items():                  # keys, d, 16-bit labels and the direction codes
        assert u.get("LDS Size", 0) >= pad * 11, (name, u)
    for name, u in sorted(usage.items()):
        print(name, u)
