"""CPU: the plain-JS statement of the surface-nets contract (js/vpt/surface.js) against the worked example and the shared arrays of
tests/golden/surface_cases.json (js/test/test_surface_host.js); and those arrays are what the numpy statement gives now."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def test_fixture_is_the_numpy_statement():
    from make_surface_fixture import cases
    from vpt_amd.surface import surface_texels
    stored = json.load(open(os.path.join(ROOT, "tests", "golden", "surface_cases.json")))
    assert stored == json.loads(json.dumps(cases()))
    names = {c['name'] for c in stored}
    assert {'r8 noise', 'r16 noise', 'rg8 channel 1', 'soft ball', 'full', 'empty'} <= names
    for c in stored:                                              # and the stored texels give the stored arrays
        shape = (c['nz'], c['ny'], c['nx']) + ((2,) if c['channels'] == 2 else ())
        a = np.array(c['texels'], np.uint8 if c['bits'] == 8 else np.uint16).reshape(shape)
        v, q = surface_texels(a, c['level'], c['channel'])
        assert v.ravel().tolist() == c['vertices'] and q.ravel().tolist() == c['quads']


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_statement():
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_surface_host.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert res.returncode == 0 and "js surface host ok" in res.stdout.decode(), res.stdout.decode()
