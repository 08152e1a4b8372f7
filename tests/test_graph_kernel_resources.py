"""CPU: every kernel of the graph unit (vpt_volume_graph.hip) compiles for gfx950 without scratch memory or register spills, with at most
64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_skeleton_kernel_resources.py).  These are conditions, not measurements (DESIGN.md "Skeleton graph" records the figures the
compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_graph_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_graph"])
    # the seed reads uint8 texels, uint16 texels and burn passes; the emitters write uint8 and uint16 texels
    counts = {"k_gr_seed": 3, "k_gr_block_sums": 1, "k_gr_scan_blocks": 1, "k_gr_classify": 1, "k_gr_init": 1, "k_gr_links": 1, "k_gr_prune": 2,
              "k_gr_classes": 2}
    for kernel, count in counts.items():
        found = [k for k in usage if re.match(r"_Z%d%s[IP]" % (len(kernel), kernel), k)]
        assert len(found) == count, (kernel, sorted(usage))
    assert len(usage) == sum(counts.values()), sorted(usage)     # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    for name, u in sorted(usage.items()):
        print(name, u)
