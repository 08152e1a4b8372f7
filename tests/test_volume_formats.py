"""CPU: the volume formats beyond R8 / RG8 / R32F / RG32F — SNORM bytes and the packed texel types (GL ES 3.0 section 3.8.3) —
on the host side: the (type, format, internalFormat) mapping of both readers, a numpy restatement of every GL decode checked against
hand-worked values, the exactness of the SNORM tap decode the kernels use, and the C-ABI / addon constants."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd.volume import device_format
from vpt_amd import readers as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (type, format, internalFormat, native format, channels in the file) of every newly accepted manifest
ACCEPTED = [
    (R.GL_BYTE, R.GL_RED, R.GL_R8_SNORM, N.FORMAT_R8_SNORM, 1),
    (R.GL_BYTE, R.GL_RG, R.GL_RG8_SNORM, N.FORMAT_RG8_SNORM, 2),
    (R.GL_BYTE, R.GL_RGB, R.GL_RGB8_SNORM, N.FORMAT_RG8_SNORM, 3),
    (R.GL_BYTE, R.GL_RGBA, R.GL_RGBA8_SNORM, N.FORMAT_RG8_SNORM, 4),
    (R.GL_UNSIGNED_SHORT_5_6_5, R.GL_RGB, R.GL_RGB565, N.FORMAT_RGB565, 1),
    (R.GL_UNSIGNED_SHORT_4_4_4_4, R.GL_RGBA, R.GL_RGBA4, N.FORMAT_RGBA4, 1),
    (R.GL_UNSIGNED_SHORT_5_5_5_1, R.GL_RGBA, R.GL_RGB5_A1, N.FORMAT_RGB5_A1, 1),
    (R.GL_UNSIGNED_INT_2_10_10_10_REV, R.GL_RGBA, R.GL_RGB10_A2, N.FORMAT_RGB10_A2, 1),
    (R.GL_UNSIGNED_INT_10F_11F_11F_REV, R.GL_RGB, R.GL_R11F_G11F_B10F, N.FORMAT_R11F_G11F_B10F, 1),
    (R.GL_UNSIGNED_INT_5_9_9_9_REV, R.GL_RGB, R.GL_RGB9_E5, N.FORMAT_RGB9_E5, 1),
]
# combinations a WebGL2 float sampler3D cannot filter (or that do not exist): the reference's error, through both readers
REJECTED = [
    (R.GL_BYTE, R.GL_RED, 0x8231),          # R8I: integer texture (isampler3D)
    (R.GL_BYTE, R.GL_RED, 33322),           # R16 (EXT_texture_norm16, not enabled by the reference)
    (R.GL_BYTE, R.GL_RG, R.GL_R8_SNORM),    # a format that does not match its internal format
    (R.GL_BYTE, R.GL_RED, R.GL_RG8_SNORM),
    (R.GL_UNSIGNED_INT_2_10_10_10_REV, R.GL_RGBA, 0x906F),   # RGB10_A2UI: integer texture
    (R.GL_UNSIGNED_SHORT_5_6_5, R.GL_RGBA, R.GL_RGB565),     # 5_6_5 is an RGB type
    (R.GL_UNSIGNED_SHORT_4_4_4_4, R.GL_RGBA, R.GL_RGB5_A1),  # type and internal format disagree
    (R.GL_UNSIGNED_INT_5_9_9_9_REV, R.GL_RGBA, R.GL_RGB9_E5),
    (R.GL_UNSIGNED_INT_10F_11F_11F_REV, R.GL_RGB, R.GL_RGB9_E5),
    (5122, R.GL_RED, 33330),                # SHORT
    (5123, R.GL_RED, 33322),                # UNSIGNED_SHORT
    (5124, R.GL_RED, 0x8235),               # INT
    (5125, R.GL_RED, 0x8236),               # UNSIGNED_INT
    (0x84FA, 0x84F9, 0x88F0),               # UNSIGNED_INT_24_8 (DEPTH_STENCIL: no 3-D depth textures in ES 3.0)
]


def modality(t, f, i):
    return {'type': t, 'format': f, 'internalFormat': i}


def test_device_format_accepts_the_filterable_snorm_and_packed_formats():
    for t, f, i, fmt, nch in ACCEPTED:
        got = device_format(modality(t, f, i))
        assert got[0] == fmt and got[1] == nch, (hex(t), hex(f), hex(i), got)
    # SNORM blocks are bytes; packed blocks are one 16- or 32-bit word per texel
    assert device_format(modality(*ACCEPTED[0][:3]))[2] == np.int8
    assert device_format(modality(*ACCEPTED[4][:3]))[2] == np.uint16
    assert device_format(modality(*ACCEPTED[7][:3]))[2] == np.uint32


def test_device_format_rejects_what_a_float_sampler_cannot_filter():
    for t, f, i in REJECTED:
        with pytest.raises(RuntimeError, match="Unknown volume datatype"):
            device_format(modality(t, f, i))


def test_existing_formats_map_as_before():
    assert device_format(modality(R.GL_UNSIGNED_BYTE, R.GL_RED, R.GL_R8))[:2] == (N.FORMAT_R8, 1)
    assert device_format(modality(R.GL_UNSIGNED_BYTE, R.GL_RGBA, R.GL_RGBA8))[:2] == (N.FORMAT_RG8, 4)
    assert device_format(modality(R.GL_FLOAT, R.GL_RED, R.GL_R32F))[:2] == (N.FORMAT_R32F, 1)
    assert device_format(modality(R.GL_HALF_FLOAT, R.GL_RGBA, 0x881A))[:2] == (N.FORMAT_RG32F, 4)


# ---- numpy restatement of the GL ES 3.0 decodes (section 3.8.3: packed types; 2.1.6.1: signed normalised) -------------------------
def snorm(c):
    """BYTE c -> max(c / 127, -1) as float32 (numpy's float32 division is correctly rounded)"""
    c = np.asarray(c).astype(np.float32)
    return np.maximum(c / np.float32(127), np.float32(-1))


def unorm(c, bits):
    return (np.asarray(c).astype(np.float32) / np.float32((1 << bits) - 1)).astype(np.float32)


def ufloat(bits, mant):
    """unsigned float with a 5-bit exponent and `mant` mantissa bits (UF11: 6, UF10: 5)"""
    bits = np.asarray(bits, dtype=np.int64)
    e, m = bits >> mant, bits & ((1 << mant) - 1)
    with np.errstate(invalid='ignore'):
        out = np.where(e == 0, m.astype(np.float64) * 2.0 ** (-14 - mant),
                       (1.0 + m / float(1 << mant)) * np.exp2(e.astype(np.float64) - 15.0))
        out = np.where(e == 31, np.where(m == 0, np.inf, np.nan), out)
    return out.astype(np.float32)


def decode_packed(words, fmt):
    """packed words -> [..., 2] float32 (r, g): what texture(uVolume, p).rg reads"""
    w = np.asarray(words).astype(np.int64)
    if fmt == N.FORMAT_RGB565:
        r, g = unorm((w >> 11) & 31, 5), unorm((w >> 5) & 63, 6)
    elif fmt == N.FORMAT_RGBA4:
        r, g = unorm((w >> 12) & 15, 4), unorm((w >> 8) & 15, 4)
    elif fmt == N.FORMAT_RGB5_A1:
        r, g = unorm((w >> 11) & 31, 5), unorm((w >> 6) & 31, 5)
    elif fmt == N.FORMAT_RGB10_A2:
        r, g = unorm(w & 1023, 10), unorm((w >> 10) & 1023, 10)
    elif fmt == N.FORMAT_R11F_G11F_B10F:
        r, g = ufloat(w & 2047, 6), ufloat((w >> 11) & 2047, 6)
    elif fmt == N.FORMAT_RGB9_E5:
        scale = np.exp2(((w >> 27) & 31).astype(np.float64) - 24.0)
        r, g = ((w & 511) * scale).astype(np.float32), (((w >> 9) & 511) * scale).astype(np.float32)
    else:
        raise ValueError(fmt)
    return np.stack([r, g], axis=-1).astype(np.float32)


def test_numpy_decodes_reproduce_hand_checked_values():
    # SNORM: -128 and -127 both read -1, 127 reads 1
    assert snorm(-128) == np.float32(-1.0) and snorm(-127) == np.float32(-1.0) and snorm(127) == np.float32(1.0) and snorm(0) == 0
    # UF11 largest finite: exponent 30, mantissa 63 -> 2^15 * (1 + 63/64) = 65024; exponent 31 -> Inf / NaN
    assert ufloat(30 << 6 | 63, 6) == np.float32(65024.0)
    assert np.isinf(ufloat(31 << 6, 6)) and np.isnan(ufloat(31 << 6 | 1, 6))
    # smallest UF10 denormal: 2^-14 / 32 = 2^-19; smallest UF11 normal 2^-14
    assert ufloat(1, 5) == np.float32(2.0 ** -19) and ufloat(1 << 6, 6) == np.float32(2.0 ** -14)
    # R11F_G11F_B10F: R in bits 10-0, G in bits 21-11 (_REV: R first); 1.0 = exponent 15, mantissa 0
    one = 15 << 6
    assert (decode_packed(one | (one << 11), N.FORMAT_R11F_G11F_B10F) == [1.0, 1.0]).all()
    # RGB9_E5: 0 -> (0, 0); all ones -> 511 * 2^(31 - 24) = 65408
    assert (decode_packed(0x00000000, N.FORMAT_RGB9_E5) == [0.0, 0.0]).all()
    assert (decode_packed(0xFFFFFFFF, N.FORMAT_RGB9_E5) == [65408.0, 65408.0]).all()
    # 5_6_5: R in bits 15-11
    assert (decode_packed(0xF800, N.FORMAT_RGB565) == [1.0, 0.0]).all() and (decode_packed(0x07E0, N.FORMAT_RGB565) == [0.0, 1.0]).all()
    assert (decode_packed(0xF000, N.FORMAT_RGBA4) == [1.0, 0.0]).all() and (decode_packed(0x07C0, N.FORMAT_RGB5_A1) == [0.0, 1.0]).all()
    # 2_10_10_10_REV: R in bits 9-0; 0x3FF / 1023 = 1, 1 / 1023 correctly rounded
    assert (decode_packed(0x3FF, N.FORMAT_RGB10_A2) == [1.0, 0.0]).all()
    assert decode_packed(1 << 10, N.FORMAT_RGB10_A2)[1] == np.float32(1) / np.float32(1023)


def test_snorm_tap_decode_is_exact_for_every_byte():
    """the kernels' tap decode fma(c, hi, c * lo) (vpt_device.h snorm_decode) equals fl32(c / 127) for every c in [-128, 255], exactly:
    computed in exact rational arithmetic with one rounding per operation, as the device does; fl32(c * fl32(1/127)) does not"""
    def f32(x):                      # x (Fraction) rounded to the nearest float32, ties to even
        f = np.float32(float(x))     # within one ulp; pick the nearest of the neighbours exactly
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))
    src = open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_device.h")).read()
    hi = np.float32(float.fromhex(re.search(r"#define VPT_SNORM_HI (\S+)f", src).group(1)))
    lo = np.float32(float.fromhex(re.search(r"#define VPT_SNORM_LO (\S+)f", src).group(1)))
    assert hi == np.float32(1.0 / 127) and lo == np.float32(1.0 / 127 - float(hi))
    wrong_recip = 0
    for c in range(-128, 256):
        want = f32(Fraction(c, 127))
        got = f32(Fraction(c) * Fraction(float(hi)) + Fraction(float(f32(Fraction(c) * Fraction(float(lo))))))
        assert got == want, c
        wrong_recip += f32(Fraction(c) * Fraction(float(hi))) != want
    assert wrong_recip == 22


def test_header_and_addon_define_the_new_formats():
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    addon = open(os.path.join(ROOT, "js", "addon", "vpt_napi.cc")).read()
    names = ["R8_SNORM", "RG8_SNORM", "RGB565", "RGBA4", "RGB5_A1", "RGB10_A2", "R11F_G11F_B10F", "RGB9_E5"]
    codes = set()
    for name in names:
        m = re.search(r"#define VPT_FORMAT_%s (\d+)" % name, header)
        assert m, name
        assert int(m.group(1)) == getattr(N, "FORMAT_" + name), name
        codes.add(int(m.group(1)))
        assert "CONST(VPT_FORMAT_%s)" % name in addon, name
    assert len(codes) == len(names) and not codes & {0, 1, 2, 3}           # the four existing codes keep their meaning


def test_js_device_format_matches_python():
    """js/vpt/Volume.js keys the same table: every accepted row maps to the same native format, every rejected one throws"""
    import shutil
    import subprocess
    import json
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not installed")
    script = r"""
const path = require('path');
const src = require('fs').readFileSync(path.join(process.argv[1], 'js/vpt/Volume.js'), 'utf8');
const R = require(path.join(process.argv[1], 'js/vpt/readers/readers.js'));
const m = { exports: {} };
const N = new Proxy({}, { get: (t, k) => k });
const req = p => p.endsWith('native.js') ? { native: () => N } : require(path.join(process.argv[1], 'js/vpt', p));
new Function('require', 'module', 'exports', src + '\nmodule.exports.deviceFormat = deviceFormat;')(req, m, m.exports);
const rows = JSON.parse(process.argv[2]);
console.log(JSON.stringify(rows.map(([t, f, i]) => { try { const d = m.exports.deviceFormat(N, { type: t, format: f, internalFormat: i }); return [d.fmt, d.channels]; }
    catch (e) { return /Unknown volume datatype/.test(e.message) ? 'raise' : e.message; } })));
"""
    rows = [list(r[:3]) for r in ACCEPTED] + [list(r) for r in REJECTED]
    res = subprocess.run([node, "-e", script, ROOT, json.dumps(rows)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert res.returncode == 0, res.stdout.decode()
    out = json.loads(res.stdout.decode().strip().splitlines()[-1])
    names = {getattr(N, k): k for k in dir(N) if k.startswith("FORMAT_")}
    for row, got in zip(ACCEPTED, out[:len(ACCEPTED)]):
        assert got == ["VPT_" + names[row[3]], row[4]], (row, got)
    assert out[len(ACCEPTED):] == ["raise"] * len(REJECTED)
