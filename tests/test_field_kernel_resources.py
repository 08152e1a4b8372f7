"""CPU: every kernel of the voxel-field unit (vpt_volume_field.hip: what the connected components and the distance transform share behind
their builders) compiles for gfx950 without scratch memory or register spills, with at most 64 KiB of LDS per workgroup and an occupancy of
at least 2: the conditions of the sibling units (tests/test_components_kernel_resources.py, tests/test_distance_kernel_resources.py, which
hold the k_pair instantiations of their units).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_field_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_field"])
    # the select emitter k_select<T>: T in {uint8_t (h), uint16_t (t)}
    emit = {k: v for k, v in usage.items() if re.match(r"_Z8k_selectI[ht]E", k)}
    assert len(emit) == 2, sorted(usage)
    # the read-back of a box of values
    plain = {k: v for k, v in usage.items() if re.match(r"_Z12k_read_fieldP", k)}
    assert len(plain) == 1, sorted(usage)
    assert len(usage) == 3, sorted(usage)                        # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
        assert u.get("LDS Size", 0) == 0, (name, u)              # plain gathers: no LDS
