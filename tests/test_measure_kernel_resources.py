"""CPU: every kernel of the measuring unit (vpt_volume_measure.hip) compiles for gfx950 without scratch memory or register spills and with
an occupancy of at least 2; the measuring kernel's LDS is exactly its table's declared size and no other kernel of the unit uses LDS: the
conditions of the sibling units (tests/test_combine_kernel_resources.py).  The instantiations are listed, so none the contract does not
admit is compiled and none escapes the conditions.  These are conditions, not measurements (DESIGN.md records the figures the compiler
reports)."""
import os
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {'h': 'uint8_t', 't': 'uint16_t'}


def declared(name):
    """the integer a `#define name value` or an enumerator of the unit gives"""
    text = open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_volume_measure.hip")).read()
    m = re.search(r"#define %s (\d+)\b" % name, text)
    if m:
        return int(m.group(1))
    words = re.search(r"enum \{ F_COUNT = 0,([^}]*)F_WORDS \}", text).group(1)
    assert name == 'F_WORDS'
    return 1 + len([w for w in words.split(',') if w.strip()])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_measure_kernels_use_no_scratch_and_the_table_is_the_lds():
    usage = resource_usage(["vpt_volume_measure"])
    # k_measure<TV, STRIDE>: the measured channel's type, the channels of its texel
    measure = {(m.group(1), int(m.group(2))): name for name in usage for m in [re.match(r"_Z9k_measureI([ht])Li([12])EE", name)] if m}
    assert set(measure) == {(t, stride) for t in TYPES for stride in (1, 2)}, sorted(measure)
    select = {m.group(1): name for name in usage for m in [re.match(r"_Z12k_select_setI([ht])E", name)] if m}
    assert set(select) == set(TYPES), sorted(select)
    init = [name for name in usage if name.startswith("_Z14k_measure_init")]
    assert len(init) == 1 and len(usage) == 7, sorted(usage)        # no kernel of the unit escapes the conditions below
    # a slot: the key, F_WORDS 32-bit words and the 64-bit sum of squares
    slots, words = declared('MS_SLOTS'), declared('F_WORDS')
    assert (slots, words) == (512, 14)
    table = slots * (4 + 4 * words + 8)
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) == (table if name in measure.values() else 0), (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
