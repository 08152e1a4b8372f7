#!/usr/bin/env python3
"""Times of the connected-components labelling on the device (vpt_volume_components and the keep / label emitters), per phase, for R8
volumes of three kinds: (a) the synthetic sphere volume thresholded at its shell, (b) uniform noise at the 6-connectivity density of the
tests (0.30: many components, the host sort matters), (c) a one-voxel-wide serpentine along z that is one component and crosses a tile face
every four voxels (the worst case of the merge).  Beside them the yardsticks taken in the same run: the device's streaming-read rate
(vpt_probe_stream_read) and the wall time of scipy.ndimage.label (where scipy is installed; else of the numpy statement) on the same array.

    python tools/components_rate.py [--out profiles/components_rates.json] [--sizes 256 512] [--connectivity 6]

The phase times are the library's own (vpt_components_profile: wall time of each phase, the stream drained at its end), the shortest of
3 runs after a warm-up by the whole call's time; keep and label are whole calls (allocation, kernel, finalize of the result) and, from the
bytes the emitters move, the rate they would need to reach if they were the whole call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd.synthetic import sphere_volume                        # noqa: E402

# bytes per voxel the streaming phases move at least (R8): flatten reads a label and the label it names; sizes reads a label; keep reads a
# texel and a rank and writes a texel; label writes two
BYTES_PER_VOXEL = {"flatten": 8, "sizes": 4, "keep": 6, "label": 7}


def serpentine(n):
    """uint8 [n][n][n]: 200 on a one-voxel-wide path, lines along z on every second row and column, joined at alternating ends"""
    s = np.zeros((n, n, n), np.uint8)                              # [x][y][z]
    end = 0
    for i0 in range(0, n, 2):
        rows = list(range(0, n, 2))
        if (i0 // 2) % 2:
            rows.reverse()
        for k, i1 in enumerate(rows):
            s[i0, i1, :] = 200
            end = n - 1 - end
            if k + 1 < len(rows):
                s[i0, (i1 + rows[k + 1]) // 2, end] = 200
        if i0 + 1 < n:
            s[i0 + 1, rows[-1], end] = 200
    return np.ascontiguousarray(s.transpose(2, 1, 0))


def cases(n):
    yield "sphere shell", sphere_volume(n, noise=48.0), 40, 120
    yield "noise 0.30", np.random.default_rng(n).integers(0, 256, size=(n, n, n)).astype(np.uint8), 0, 76
    yield "serpentine", serpentine(n), 200, 200


def host_label(a, lo, hi, connectivity):
    try:
        from scipy import ndimage
    except ImportError:
        t0 = time.perf_counter()
        count = len(vpt_amd.components_texels(a, lo, hi, connectivity)[1])
        return "numpy statement", time.perf_counter() - t0, count
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    t0 = time.perf_counter()
    _, count = ndimage.label((a >= lo) & (a <= hi), structure=structure)
    return "scipy.ndimage.label", time.perf_counter() - t0, int(count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--connectivity", type=int, default=6)
    ap.add_argument("--no-host", action="store_true", help="skip the host labelling")
    a = ap.parse_args()
    ctx = vpt_amd.Context(0)
    probe = ctx.stream_read_rate(1 << 30, 5)
    out = {"stream_read_GB_per_s": probe, "connectivity": a.connectivity, "bytes_per_voxel": BYTES_PER_VOXEL, "cases": {}}
    for n in a.sizes:
        for name, vol, lo, hi in cases(n):
            src = vpt_amd.Volume.from_array(ctx, vol)
            best = None
            for run in range(4):
                ctx.synchronize()
                t0 = time.perf_counter()
                found = src.components(lo, hi, a.connectivity)
                whole = time.perf_counter() - t0
                phases, merges, flattens = found.profile()
                if run and (best is None or whole < best[0]):
                    best = (whole, phases, merges, flattens, found.info)
                if run < 3:
                    found.destroy()
            whole, phases, merges, flattens, info = best
            row = {"whole_call_ms": whole * 1e3, "phases_ms": phases, "merge_launches": merges, "flatten_launches": flattens, "info": info}
            for emitter, call in (("keep", lambda: found.keep(1, 1)), ("label", found.label)):
                times = []
                for _ in range(4):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    v = call()
                    ctx.synchronize()
                    times.append(time.perf_counter() - t0)
                    v.destroy()
                row[emitter + "_call_ms"] = min(times[1:]) * 1e3
            found.destroy()
            src.destroy()
            voxels = float(n) ** 3
            for phase in ("flatten", "sizes"):
                launches = flattens if phase == "flatten" else 1
                if phases[phase] > 0:
                    rate = BYTES_PER_VOXEL[phase] * voxels * max(launches, 1) / (phases[phase] * 1e-3) / 1e9
                    row[phase + "_GB_per_s"] = rate
                    row[phase + "_fraction_of_stream_read"] = rate / probe
            for emitter in ("keep", "label"):
                rate = BYTES_PER_VOXEL[emitter] * voxels / (row[emitter + "_call_ms"] * 1e-3) / 1e9
                row[emitter + "_call_GB_per_s"] = rate
                row[emitter + "_call_fraction_of_stream_read"] = rate / probe
            if not a.no_host:
                what, seconds, count = host_label(vol, lo, hi, a.connectivity)
                row["host"] = {"what": what, "ms": seconds * 1e3, "components": count}
            out["cases"]["%d^3 %s" % (n, name)] = row
            del vol
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
