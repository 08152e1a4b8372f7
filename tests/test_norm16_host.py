"""CPU: the 16-bit normalised formats (EXT_texture_norm16) on the host side — the opt-in manifest mapping of Python and Node.js, the
combinations that keep raising, the C ABI / Python / addon constants, and the exactness of the tap decode the kernels use (checked for every
16-bit value in exact rational arithmetic)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.context import Context
from vpt_amd.volume import device_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (type, format, internalFormat, native format, channels in the file, block dtype)
NORM16 = [
    (R.GL_UNSIGNED_SHORT, R.GL_RED, 0x822A, N.FORMAT_R16, 1, np.uint16),
    (R.GL_UNSIGNED_SHORT, R.GL_RG, 0x822C, N.FORMAT_RG16, 2, np.uint16),
    (R.GL_UNSIGNED_SHORT, R.GL_RGB, 0x8054, N.FORMAT_RG16, 3, np.uint16),
    (R.GL_UNSIGNED_SHORT, R.GL_RGBA, 0x805B, N.FORMAT_RG16, 4, np.uint16),
    (R.GL_SHORT, R.GL_RED, 0x8F98, N.FORMAT_R16_SNORM, 1, np.int16),
    (R.GL_SHORT, R.GL_RG, 0x8F99, N.FORMAT_RG16_SNORM, 2, np.int16),
    (R.GL_SHORT, R.GL_RGB, 0x8F9A, N.FORMAT_RG16_SNORM, 3, np.int16),
    (R.GL_SHORT, R.GL_RGBA, 0x8F9B, N.FORMAT_RG16_SNORM, 4, np.int16),
]
# SHORT / UNSIGNED_SHORT combinations that raise with the extension or without it: integer formats, mismatched triples, other types' formats
STILL_REJECTED = [
    (R.GL_UNSIGNED_SHORT, R.GL_RED, 0x8234),          # R16UI
    (R.GL_SHORT, R.GL_RED, 0x8233),                   # R16I
    (R.GL_UNSIGNED_SHORT, R.GL_RG, 0x823A),           # RG16UI
    (R.GL_UNSIGNED_SHORT, 0x8D94, 0x8234),            # RED_INTEGER
    (R.GL_SHORT, R.GL_RED, 0x822A),                   # SHORT with a UNORM format
    (R.GL_UNSIGNED_SHORT, R.GL_RED, 0x8F98),          # UNSIGNED_SHORT with an SNORM format
    (R.GL_UNSIGNED_SHORT, R.GL_RG, 0x822A),           # format and internal format disagree
    (R.GL_UNSIGNED_SHORT, R.GL_RED, 0x822C),
    (R.GL_SHORT, R.GL_RGBA, 0x8F9A),
    (R.GL_UNSIGNED_SHORT, R.GL_RED, 33330),           # R16F
    (R.GL_UNSIGNED_SHORT, R.GL_RED, R.GL_R8),
    (R.GL_UNSIGNED_SHORT, 0x1902, 0x81A5),            # DEPTH_COMPONENT16
    (R.GL_BYTE, R.GL_RED, 0x822A),
    (5125, R.GL_RED, 0x822A),                         # UNSIGNED_INT
]


def modality(t, f, i):
    return {'type': t, 'format': f, 'internalFormat': i}


def host_context():
    """a Context without a device (getExtension is pure host state)"""
    c = Context.__new__(Context)
    c._extensions = {}
    return c


def test_extension_object_like_webgl():
    c = host_context()
    assert c.getExtension('OES_texture_float_linear_nonexistent') is None
    assert c.getExtension('WEBGL_lose_context') is None
    assert not c.extension_enabled('EXT_texture_norm16')
    ext = c.getExtension('EXT_texture_norm16')
    assert ext and c.extension_enabled('EXT_texture_norm16')
    assert c.getExtension('EXT_texture_norm16') is ext
    assert (ext.R16_EXT, ext.RG16_EXT, ext.RGB16_EXT, ext.RGBA16_EXT) == (0x822A, 0x822C, 0x8054, 0x805B)
    assert (ext.R16_SNORM_EXT, ext.RG16_SNORM_EXT, ext.RGB16_SNORM_EXT, ext.RGBA16_SNORM_EXT) == (0x8F98, 0x8F99, 0x8F9A, 0x8F9B)
    assert not host_context().extension_enabled('EXT_texture_norm16')       # an enabled extension belongs to its context


def test_mapping_with_and_without_the_extension():
    on, off = host_context(), host_context()
    on.getExtension('EXT_texture_norm16')
    for t, f, i, fmt, nch, dt in NORM16:
        assert device_format(modality(t, f, i), on) == (fmt, nch, dt), (t, hex(f), hex(i))
        for gl in (None, off):
            with pytest.raises(RuntimeError, match="Unknown volume datatype"):
                device_format(modality(t, f, i), gl)
        with pytest.raises(RuntimeError, match="Unknown volume datatype"):
            device_format(modality(t, f, i))                              # the one-argument call keeps raising
    for t, f, i in STILL_REJECTED:
        for gl in (None, off, on):
            with pytest.raises(RuntimeError, match="Unknown volume datatype"):
                device_format(modality(t, f, i), gl)
    # the other formats map as they did, with the extension or without it
    for gl in (None, on):
        assert device_format(modality(R.GL_UNSIGNED_BYTE, R.GL_RED, R.GL_R8), gl)[:2] == (N.FORMAT_R8, 1)
        assert device_format(modality(R.GL_FLOAT, R.GL_RG, 0x8230), gl)[:2] == (N.FORMAT_RG32F, 2)
        assert device_format(modality(R.GL_BYTE, R.GL_RED, R.GL_R8_SNORM), gl)[:2] == (N.FORMAT_R8_SNORM, 1)


def test_node_tables_match():
    """js/vpt/Volume.js and the reader constants carry the same table, behind the context's getExtension"""
    vol = open(os.path.join(ROOT, "js", "vpt", "Volume.js")).read()
    readers = open(os.path.join(ROOT, "js", "vpt", "readers", "readers.js")).read()
    consts = dict((m.group(1), int(m.group(2), 0)) for m in re.finditer(r"(GL_\w+_EXT|GL_UNSIGNED_SHORT|GL_SHORT) = (0x[0-9A-Fa-f]+|\d+)", readers))
    assert consts['GL_UNSIGNED_SHORT'] == 5123 and consts['GL_SHORT'] == 5122
    names = {1: '', 2: 'RG', 3: 'RGB', 4: 'RGBA'}
    for t, f, i, fmt, nch, dt in NORM16:
        ifmt = 'GL_%s16%s_EXT' % (names[nch] or 'R', '_SNORM' if dt == np.int16 else '')
        assert consts[ifmt] == i, ifmt
        cname = {N.FORMAT_R16: 'VPT_FORMAT_R16', N.FORMAT_RG16: 'VPT_FORMAT_RG16', N.FORMAT_R16_SNORM: 'VPT_FORMAT_R16_SNORM',
                 N.FORMAT_RG16_SNORM: 'VPT_FORMAT_RG16_SNORM'}[fmt]
        assert "R.%s, R.%s, '%s', %d" % ('GL_SHORT' if dt == np.int16 else 'GL_UNSIGNED_SHORT', ifmt, cname, nch) in \
            vol.replace("GL_RED, ", "").replace("GL_RG, ", "").replace("GL_RGB, ", "").replace("GL_RGBA, ", ""), (ifmt, cname)
    assert "extensionEnabled('EXT_texture_norm16')" in vol
    ctx = open(os.path.join(ROOT, "js", "vpt", "Context.js")).read()
    assert "getExtension(name)" in ctx and "EXT_texture_norm16" in ctx


def test_header_native_and_addon_constants():
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    consts = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define (VPT_FORMAT_\w+)\s+(\d+)", header))
    want = {"VPT_FORMAT_R16": 12, "VPT_FORMAT_RG16": 13, "VPT_FORMAT_R16_SNORM": 14, "VPT_FORMAT_RG16_SNORM": 15}
    for k, v in want.items():
        assert consts[k] == v and getattr(N, k[4:]) == v, k
    # the existing codes do not move
    assert [consts["VPT_FORMAT_" + k] for k in ("R8", "RG8", "R32F", "RG32F", "R8_SNORM", "RG8_SNORM", "RGB9_E5")] == [0, 1, 2, 3, 4, 5, 11]
    for k, v in consts.items():
        assert getattr(N, k[4:]) == v, k
    addon = open(os.path.join(ROOT, "js", "addon", "vpt_napi.cc")).read()
    for name in want:
        assert "CONST(%s)" % name in addon, name
    device = open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_variants.h")).read()
    assert re.search(r"#define VPT_V_NORM16\s+512\b", device)


# ---- the tap decode: exact in rational arithmetic for every 16-bit value ---------------------------------------------------------
def round_f32(q):
    """the float32 nearest to the rational q (ties to even), as a Fraction (normal range: the values here are in [2^-16, 1])"""
    if q == 0:
        return Fraction(0)
    s = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    m = q / Fraction(2) ** (e - 23)
    n, r = divmod(m.numerator, m.denominator)
    r = Fraction(r, m.denominator)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2):
        n += 1
    return s * n * Fraction(2) ** (e - 23)


def constant(device, name):
    m = re.search(r"#define %s (0x1\.([0-9a-f]+)p(-?\d+))f" % name, device)
    assert m, name
    return Fraction(int("1" + m.group(2), 16), 16 ** len(m.group(2))) * Fraction(2) ** int(m.group(3))


@pytest.mark.parametrize("signed", [False, True])
def test_split_decode_is_exact_for_every_value(signed):
    """fma(c, HI, fl32(c * LO)) == fl32(c / N) for every c the storage can hold (N = 65535, or 32767 with -32768 clamped to -32767);
    fl32(c * fl32(1/N)) is not (512 and 1536 values); numpy's float32(c / N) in float64 is exact (the tests' R32F twins use it)"""
    device = open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_device.h")).read()
    p = "VPT_SNORM16" if signed else "VPT_UNORM16"
    hi, lo = constant(device, p + "_HI"), constant(device, p + "_LO")
    n = 32767 if signed else 65535
    assert hi == round_f32(Fraction(1, n)) and lo == round_f32(Fraction(1, n) - hi)
    values = range(-32767, 32768) if signed else range(65536)
    numpy_f32 = (np.array(values, np.float64) / n).astype(np.float32)
    wrong_mul = 0
    for k, c in enumerate(values):
        exact = round_f32(Fraction(c, n))
        assert round_f32(c * hi + round_f32(c * lo)) == exact, c
        assert Fraction(float(numpy_f32[k])) == exact, c
        wrong_mul += round_f32(c * hi) != exact
    assert wrong_mul == (1536 if signed else 512)
