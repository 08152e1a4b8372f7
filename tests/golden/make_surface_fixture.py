#!/usr/bin/env python3
"""Writes tests/golden/surface_cases.json: small volumes with the vertices, quads and info vpt_amd.surface.surface_texels gives for them.
js/test/test_surface_host.js holds the plain-JS statement to these arrays; tests/test_js_surface_host.py holds the file to the numpy
statement as it is now.  Run from the repository root: python tests/golden/make_surface_fixture.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vpt_amd.surface import surface_texels  # noqa: E402


def cases():
    rng = np.random.default_rng(2027)
    r8 = rng.integers(0, 256, (5, 7, 9), dtype=np.uint8)
    r16 = rng.integers(0, 65536, (4, 5, 6), dtype=np.uint16)
    r16[1, 2, 3] = 65535
    rg8 = rng.integers(0, 256, (3, 4, 5, 2), dtype=np.uint8)
    z, y, x = np.indices((7, 8, 9)).astype(np.float64)
    ball = np.clip(np.rint(128 + 60 * (2.6 - np.sqrt((x - 4) ** 2 + (y - 3.5) ** 2 + (z - 3) ** 2))), 0, 255).astype(np.uint8)
    out = []
    for name, a, level, channel in (('r8 noise', r8, 128, 0), ('r8 noise level 1', r8, 1, 0), ('r8 noise level 255', r8, 255, 0),
                                    ('r16 noise', r16, 30000, 0), ('r16 noise level 65535', r16, 65535, 0), ('rg8 channel 1', rg8, 99, 1),
                                    ('soft ball', ball, 128, 0), ('full', np.full((2, 3, 4), 255, np.uint8), 1, 0),
                                    ('empty', np.full((2, 3, 4), 7, np.uint8), 8, 0)):
        info = {}
        v, q = surface_texels(a, level, channel, info=info)
        out.append({'name': name, 'bits': 8 * a.dtype.itemsize, 'channels': 2 if a.ndim == 4 else 1, 'nx': a.shape[2], 'ny': a.shape[1], 'nz': a.shape[0],
                    'level': level, 'channel': channel, 'texels': a.ravel().tolist(), 'vertices': v.ravel().tolist(), 'quads': q.ravel().tolist(),
                    'info': info})
    return out


if __name__ == '__main__':
    with open(os.path.join(ROOT, 'tests', 'golden', 'surface_cases.json'), 'w') as f:
        json.dump(cases(), f, separators=(',', ':'))
        f.write('\n')
