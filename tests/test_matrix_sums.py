"""CPU: the host-computed constant part of inverseMvp * (x, y, -+1, 1) (vpt_mat4_sums.h; PassArgs.mvp_near / mvp_far).  The kernels used to start
each component of the product with fma(m[8+i], -+1, m[12+i]); the host now passes m[12+i] - m[8+i] and m[12+i] + m[8+i].  Both round the
exact sum once, so the bits must be equal — for a few hundred random matrices and for entries that are infinite, zero (of either sign),
denormal or at the ends of the float range.  The fma is restated in numpy: float32 operands are exact in float64, the sum of two of them is
exact there unless their exponents lie more than 29 binades apart — then and only then the float64 sum is itself rounded, and the pair is
compared through the exact integer sum instead."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vpt_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "vpt_mat4_sums.h"
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    float m[16], sums[8];
    while (fread(m, sizeof(float), 16, in) == 16) {
        mat4_point_sums(m, sums, sums + 4);
        fwrite(sums, sizeof(float), 8, out);
    }
    fclose(in); fclose(out);
    return 0;
}
"""


def matrices():
    rng = np.random.default_rng(20)
    ms = [rng.standard_normal((300, 16)).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 7, (300, 1)).astype(np.float32)]
    # random bit patterns: every exponent, denormals, infinities and NaNs among them
    ms.append(rng.integers(0, 2 ** 32, (300, 16), dtype=np.uint64).astype(np.uint32).view(np.float32))
    tiny, huge = np.float32(1e-45), np.finfo(np.float32).max
    special = np.float32([np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, np.float32(1.1754942e-38), huge, -huge, 1.0, -1.0, np.float32(2 ** -24), 16777216.0, 3.0])
    pairs = np.float32([(a, b) for a in special for b in special])
    m = np.zeros((len(pairs), 16), np.float32)
    m[:, 8:12] = pairs[:, :1]; m[:, 12:16] = pairs[:, 1:]
    ms.append(m)
    return np.concatenate(ms)


def fma_sign(m8, z, m12):
    """fmaf(m8, z, m12) for z = -+1 with one rounding, in numpy: the product is exact, the sum is rounded once to float32"""
    with np.errstate(invalid="ignore"):                         # (signalling NaNs among the random bit patterns)
        a, b = (m8.astype(np.float64) * z), m12.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b                                               # exact in float64 when the exponents are close enough ...
        out = s.astype(np.float32)
    fin = np.isfinite(a) & np.isfinite(b) & (a != 0) & (b != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        far = fin & (np.abs(np.log2(np.abs(a)) - np.log2(np.abs(b))) > 28)
    for i in np.argwhere(far):                                  # ... else through the exact rational sum, rounded once
        i = tuple(i)
        exact = Fraction(float(a[i])) + Fraction(float(b[i]))
        out[i] = round_once(exact)
    return out


def round_once(x):
    """the float32 nearest to the rational x, ties to even (numpy rounds a float64 the same way; x is first brought exactly into reach)"""
    lo = np.float32(float(x))                                   # float(x) rounds to float64, then to float32: a candidate next to the answer
    best = None
    with np.errstate(over="ignore"):
        near = (np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf)))
    for c in near:
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - x)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, c, even)
    big = Fraction(float(np.finfo(np.float32).max)) + Fraction(2) ** 103   # halfway to 2^128: rounds to infinity
    if abs(x) >= big:
        return np.float32(np.inf if x > 0 else -np.inf)
    return best[1]


def test_host_sums_equal_the_fma_with_unit_z(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "sums.cc", tmp_path / "sums"
    src.write_text(PROGRAM)
    # (optimised, with contraction allowed: the header's volatile operands must make that irrelevant)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=fast", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    m = matrices()
    (tmp_path / "in.bin").write_bytes(m.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(len(m), 8)
    for z, cols in ((-1.0, got[:, :4]), (1.0, got[:, 4:])):
        want = fma_sign(m[:, 8:12], z, m[:, 12:16])
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(cols), nan), "z = %g: NaNs elsewhere" % z
        bad = (cols.view(np.uint32) != want.view(np.uint32)) & ~nan
        assert not bad.any(), (z, m[np.argwhere(bad)[0][0]], cols[bad][:4], want[bad][:4])
