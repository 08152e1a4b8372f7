"""CPU: the quasi-cubic filter's host side — the C ABI constant, the Python and Node.js constants and filter-name mappings — and the
weight identities of the contract's reference implementation (the fixture generator's qc_weight, which tests/test_gpu_quasicubic.py's
numpy restatement follows)."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd.volume import filter_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def test_header_native_and_addon_agree():
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    consts = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define (VPT_FILTER_\w+)\s+(\d+)", header))
    assert consts == {"VPT_FILTER_NEAREST": 0, "VPT_FILTER_LINEAR": 1, "VPT_FILTER_QUASI_CUBIC": 2}, consts
    assert (N.FILTER_NEAREST, N.FILTER_LINEAR, N.FILTER_QUASI_CUBIC) == (0, 1, 2)
    addon = open(os.path.join(ROOT, "js", "addon", "vpt_napi.cc")).read()
    for name in consts:
        assert "CONST(%s)" % name in addon, name
    device = open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_variants.h")).read()
    assert re.search(r"#define VPT_V_QCUBIC\s+256\b", device)


def test_filter_names():
    assert filter_code('linear') == N.FILTER_LINEAR
    assert filter_code('nearest') == N.FILTER_NEAREST
    assert filter_code('quasicubic') == N.FILTER_QUASI_CUBIC
    for other in ('cubic', 'QuasiCubic', 'quasi-cubic', '', None, 2, 'LINEAR'):     # Volume.js:121: anything else is NEAREST
        assert filter_code(other) == N.FILTER_NEAREST, other


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_filter_mapping_is_the_same():
    names = ['linear', 'nearest', 'quasicubic', 'cubic', '']
    script = ("const { filterCode } = require(%r); const N = { VPT_FILTER_NEAREST: 0, VPT_FILTER_LINEAR: 1, VPT_FILTER_QUASI_CUBIC: 2 };"
              "console.log(JSON.stringify(%s.map(f => filterCode(N, f))));") % (os.path.join(ROOT, "js", "vpt", "Volume.js"), json.dumps(names))
    res = subprocess.run(["node", "-e", script], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert res.returncode == 0, res.stdout.decode()
    assert json.loads(res.stdout.decode().strip().splitlines()[-1]) == [filter_code(n) for n in names]


def test_weight_identities():
    from make_quasicubic_fixture import qc_weight
    for f, want in ((0.0, 0.0), (0.5, 0.5), (1.0, 1.0)):
        got = qc_weight(np.float32(f))
        assert isinstance(got, np.float32)
        assert got.view(np.uint32) == np.float32(want).view(np.uint32), (f, got)
    # smooth, monotone and symmetric about 1/2 on a grid of weights: f' + (1 - f)' == 1 within rounding
    f = np.linspace(0, 1, 4097, dtype=np.float32)
    w = np.array([qc_weight(x) for x in f])
    assert (np.diff(w) >= 0).all()
    assert np.abs(w + w[::-1] - 1).max() < 4e-7
