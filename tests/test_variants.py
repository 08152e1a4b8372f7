"""CPU: the one switch from a run-time sampler variant to a template argument (vpt_amd/csrc/vpt_variants.h), compiled with the host
compiler alone and run over every value in [0, 2048): the sampler form accepts exactly the variants that exist —
{32-bit, wide tables} x {LINEAR, NEAREST, QUASI_CUBIC} x {R, RG} x {u8, f32, s8, u16, s16} = 60 — and hands each to the callable as the
compile-time constant of the same value; the two bit-set forms (the tile-class kernels, the MISS-tile kernels of the volume formats) accept
exactly the subsets of their bits; every other value is refused (no value falls through to some default kernel)."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vpt_amd", "csrc")
LIMIT = 2048

PROGRAM = r"""
#include "vpt_variants.h"
#include <cstdio>
static_assert(sampler_variant_valid(0) && !sampler_variant_valid(VPT_V_NEAREST | VPT_V_QCUBIC), "the predicate is a constant expression");
struct Seen { template <int V> int operator()(std::integral_constant<int, V>) const { return V; } };   // the V the callable was given
static int refused() { return -1; }
int main() {
    for (int v = 0; v < %d; v++)
        std::printf("%%d %%d %%d %%d\n", v, dispatch_sampler_variant(v, Seen{}, refused),
                    dispatch_variant<VPT_V_WIDE | VPT_V_FAST | VPT_V_REC>(v, Seen{}, refused),
                    dispatch_variant<VPT_V_NEAREST | VPT_V_RG | VPT_V_F32>(v, [](auto V) { return (int)decltype(V)::value; }, refused));
    return 0;
}
""" % LIMIT


def bits():
    text = open(os.path.join(CSRC, "vpt_variants.h")).read()
    return dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define VPT_V_([A-Z0-9]+)\s+(\d+)\b", text))


def subsets(*values):
    return {sum(c) for n in range(len(values) + 1) for c in itertools.combinations(values, n)}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("variants") / "variants")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-x", "c++", "-", "-o", exe], input=PROGRAM.encode(), check=True)
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.check_output([exe]).decode().splitlines()]
    assert [r[0] for r in rows] == list(range(LIMIT))
    return rows


def test_bits_are_distinct_and_where_the_kernel_names_expect_them():
    b = bits()
    assert b == {"WIDE": 1, "NEAREST": 2, "ALIGNED": 4, "RG": 8, "FAST": 16, "F32": 32, "REC": 64, "SNORM": 128, "QCUBIC": 256, "NORM16": 512}, b
    assert max(b.values()) * 2 <= LIMIT


def test_sampler_dispatch_accepts_exactly_the_sixty_variants(table):
    b = bits()
    want = {wide | filt | channels | texels
            for wide in (0, b["WIDE"])
            for filt in (0, b["NEAREST"], b["QCUBIC"])                       # LINEAR, NEAREST, QUASI_CUBIC
            for channels in (0, b["RG"])
            for texels in (0, b["F32"], b["SNORM"], b["NORM16"], b["NORM16"] | b["SNORM"])}   # u8, f32, s8, u16, s16
    assert len(want) == 60
    accepted = {v for v, seen, _, _ in table if seen != -1}
    assert accepted == want, (sorted(accepted - want), sorted(want - accepted))
    for v, seen, _, _ in table:
        assert seen == (v if v in want else -1), (v, seen)


def test_bit_set_dispatch_accepts_exactly_the_subsets_of_its_bits(table):
    b = bits()
    classes = subsets(b["WIDE"], b["FAST"], b["REC"])
    formats = subsets(b["NEAREST"], b["RG"], b["F32"])
    assert len(classes) == 8 and len(formats) == 8
    for v, _, cls, fmt in table:
        assert cls == (v if v in classes else -1), (v, cls)
        assert fmt == (v if v in formats else -1), (v, fmt)
