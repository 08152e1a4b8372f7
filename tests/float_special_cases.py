"""Float volumes with a special texel at a CHOSEN position, shared by tests/test_float_special_cases.py (CPU: the conditions the cases must
meet, on the oracle alone) and tests/test_gpu_float_specials.py (GPU: probe_sample and the renderers against the oracle, bit for bit).

Why positions matter.  GL's LINEAR filter (the oracle's linear_coord) clamps the two tap INDICES of the unclamped u = s N - 0.5; the brick
sampler clamps u into [0, N - 1] first and takes cell (i, i + 1) with weight 0 where u was below 0.  lerp(t0, t1, 0) = fma(0, t1 - t0, t0) is
t0 only while t1 - t0 is finite, so the two differ exactly where, along some axis, texel 0 is finite and texel 1 is infinite, NaN, or finite
with a difference that overflows, for every sample below that axis's first texel centre (or outside the cube on the low side, or with a NaN
coordinate).  On the high side the bricks' apron repeats t[N - 1]: both blend a texel with itself.  clamp_first() below is the numpy
statement of the clamp-first formula WITHOUT the second-tap select the float sampler carries (vpt_device.h below_first): deliberately wrong,
kept so that the CPU test can prove that the cases tell the two apart at index 1 and nowhere else.

A case is one volume: finite noise in [0.2, 0.9] with one special texel, or one pair, whose index along the axis under test is one of
0, 1, 3, 4, N - 2, N - 1 and whose other two indices are >= 2 where the axis has them (so that only the axis under test can show the clamp).
Specials: nan, +inf, -inf; `overflow`, the finite pair 3e38 | -3e38 on texels (index - 1, index) ((0, 1) reversed for index 0); `large`, the
pair -0.9e37 | 0.9e37 just under the boundary atlas's threshold (k_scan_finite: 1e37), which keeps the atlas on and can never differ.  The
pair's order matters to what a test can SEE: with texel 0 = 3e38 the contract's sample below the first texel centre looks up the transfer
function's last entry and the clamp-first NaN its entry 0; the other way round (the index-0 case) -3e38 looks up entry 0 as the NaN does, so
that case shows nothing in the colour.  "The index-1 case" is thus index 1 for every special but `large`.  One more case has texels 0 and 1
both special (+inf, nan): both statements give NaN.

The transfer function's entry 0 (row 0 and column 0 of the two-channel one) is white and opaque and every other entry is at most 200: a NaN
sample looks up entry 0, which no value of the noise reaches, so a poisoned sample shows in the colour.

Probe points per case: the coordinate on the axis under test walks -inf, -0.25, -1e-7, 0, 0.25/N, 0.5/N and its two float neighbours, every
texel centre, every cell border, 1 - 0.25/N, 1, 1 + 1e-7, 1.25, +inf, NaN; the other two axes take ten positions each (outside and just
inside their own low edge, five within 0.3 texels of the special texel's centre — the overflowing pair poisons a sample only where the
special texels' combined weight on those axes exceeds 0.57 —, two drawn, one beyond the high edge)."""
import ctypes as C
import functools

import numpy as np

F = np.float32
FILTERS = ("nearest", "linear", "quasicubic")
MAIN = (7, 6, 9)                                       # (nz, ny, nx): every axis >= 6, x crosses two brick borders
SHORT = ((2, 1, 8), (1, 8, 2))                         # axes of 1 and 2 texels; 8: 0.5 / N lands on u == 0 exactly
SPECIALS = {"nan": (np.nan,), "+inf": (np.inf,), "-inf": (-np.inf,), "overflow": (3e38, -3e38), "large": (-0.9e37, 0.9e37)}
TF_WIDTH, TF_ROWS = 16, 8


def transfer_function(channels):
    rng = np.random.default_rng(41)
    tf = rng.integers(0, 201, size=(TF_ROWS if channels == 2 else 1, TF_WIDTH, 4), dtype=np.uint8)
    tf[:, 0] = 255
    if channels == 2:
        tf[0, :] = 255
    return tf


class Case:
    def __init__(self, name, texels, axis, index, special, channel, differs):
        self.name, self.texels, self.axis, self.index, self.special, self.channel, self.differs = name, texels, axis, index, special, channel, differs
        self.channels = 2 if texels.ndim == 4 else 1
        self.dims = texels.shape[:3]
        self.tf = transfer_function(self.channels)
        self.main = self.dims == MAIN
        self.atlas = special == "large"                # every texel finite and below the threshold: the boundary atlas stays in use

    def __repr__(self):
        return self.name

    @functools.cached_property
    def points(self):
        return probe_points(self)


def indices(n):
    return sorted({i for i in (0, 1, 3, 4, n - 2, n - 1) if 0 <= i < n})


def _size(dims, axis):
    return dims[2 - axis]                              # axis 0 = x = the last array axis


def _other_index(rng, n):
    return int(rng.integers(2, n)) if n >= 3 else 0


def _place(channel_view, axis, at, others, value):
    pos = list(others)
    pos[axis] = at
    channel_view[pos[2], pos[1], pos[0]] = value


def _one(dims, channels, channel, axis, index, special, seed):
    rng = np.random.default_rng(seed)
    shape = dims + ((2,) if channels == 2 else ())
    texels = rng.uniform(0.2, 0.9, size=shape).astype(F)
    view = texels[..., channel] if channels == 2 else texels
    n = _size(dims, axis)
    others = [_other_index(rng, _size(dims, a)) for a in range(3)]
    values = SPECIALS[special]
    if len(values) == 1:
        _place(view, axis, index, others, values[0])
        differs = index == 1
    else:
        lo, hi = (index - 1, index) if index >= 1 else (1, 0)
        _place(view, axis, lo, others, values[0]); _place(view, axis, hi, others, values[1])
        differs = special == "overflow" and index == 1
    name = "%s-%dx%dx%d-%s%s-%s-%d" % ("rg32f" if channels == 2 else "r32f", dims[2], dims[1], dims[0], "xyz"[axis],
                                       "-ch%d" % channel if channels == 2 else "", special, index)
    return Case(name, texels, axis, index, special, channel, differs), others


@functools.lru_cache(maxsize=None)
def cases():
    out, seed = [], 0
    for axis in range(3):
        for special in SPECIALS:
            for k, index in enumerate(indices(_size(MAIN, axis))):
                seed += 1
                out.append(_one(MAIN, 1, 0, axis, index, special, seed)[0])
                # RG32F: the channel alternates along the indices, index 1 in both channels
                for channel in ((0, 1) if index == 1 else (k % 2,)):
                    seed += 1
                    out.append(_one(MAIN, 2, channel, axis, index, special, seed)[0])
    for dims in SHORT:
        for axis in range(3):
            n = _size(dims, axis)
            for special in SPECIALS:
                if n < 2 and len(SPECIALS[special]) == 2:
                    continue
                for index in indices(n):
                    seed += 1
                    out.append(_one(dims, 1, 0, axis, index, special, seed)[0])
    # texels 0 and 1 of x both special: +inf beside nan
    c, others = _one(MAIN, 1, 0, 0, 0, "+inf", 9001)
    _place(c.texels, 0, 1, others, np.nan)
    c.name, c.special = "r32f-9x6x7-x-both-0", "both"
    out.append(c)
    return tuple(out)


def _axis_walk(n):
    h = F(0.5) / F(n)
    v = [-np.inf, -0.25, -1e-7, 0.0, 0.25 / n, h, np.nextafter(h, F(-1)), np.nextafter(h, F(2))]
    v += [(k + 0.5) / n for k in range(n)] + [k / n for k in range(1, n)]
    v += [1 - 0.25 / n, 1.0, 1 + 1e-7, 1.25, np.inf, np.nan]
    return np.array(v, F)


def probe_points(case):
    """[points][3] float32 (x, y, z)"""
    rng = np.random.default_rng(7 + case.axis)
    special = np.argwhere(~(np.abs(case.texels) < 1.0))[0]            # (z, y, x[, channel]) of a special texel
    per_axis = []
    for a in range(3):
        n = _size(case.dims, a)
        if a == case.axis:
            per_axis.append(_axis_walk(n))
            continue
        c = (special[2 - a] + 0.5) / n
        per_axis.append(np.array([-0.25, 0.25 / n, c, c - 0.1 / n, c + 0.1 / n, c - 0.3 / n, c + 0.3 / n, rng.uniform(0, 1), rng.uniform(0, 1), 1.25], F))
    x, y, z = np.meshgrid(*per_axis, indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3), dtype=F)


# ---- the expected value: the oracle ----------------------------------------------------------------------------------------------------------
_expected = {}


def oracle_colours(oracle, texels, filt, tf, points):
    sc = oracle.OracleScene(texels, filt, tf=tf)
    p = np.ascontiguousarray(points, F)
    out = np.empty((p.shape[0], 4), F)
    oracle.lib().vpo_sample_volume_colors(C.byref(sc.c), p.ctypes.data_as(C.c_void_p), p.shape[0], out.ctypes.data_as(C.c_void_p))
    return out


def expected(oracle, case, filt):
    """vpo_sample_volume_color at the case's points -> [points][4] float32; computed once, read-only"""
    key = (case.name, filt)
    if key not in _expected:
        out = oracle_colours(oracle, case.texels, filt, case.tf, case.points)
        out.setflags(write=False)
        _expected[key] = out
    return _expected[key]


# ---- the deliberately wrong statement: clamp u first, blend (t[i], t[i + 1]) with weight 0 ---------------------------------------------------
def fmaf(a, b, c):
    """fl32(a * b + c) with one rounding, vectorised: the product of two floats is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the error's sign), which a final rounding to 24 bits cannot tell from the exact sum (53 >= 24 + 2)"""
    a, b, c = np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def lerpf(a, b, f):
    with np.errstate(invalid="ignore", over="ignore"):
        return fmaf(f, (np.asarray(b, F) - np.asarray(a, F)).astype(F), a)


def qc_weight(f):
    return ((f * f).astype(F) * (F(3) - (F(2) * f).astype(F))).astype(F)


def _clamped_cell(s, n):
    """linear_cell: u = med3(fma(s, N, -0.5), 0, N - 1) (a NaN gives 0), i = trunc(u), f = fract(u); the second tap is the apron's"""
    u = fmaf(s, F(n), F(-0.5))
    with np.errstate(invalid="ignore"):
        u = np.where(np.isnan(u), F(0), np.clip(u, F(0), F(n - 1))).astype(F)
    i = u.astype(np.int64)
    return i, np.minimum(i + 1, n - 1), (u - np.floor(u)).astype(F)


def _index_clamped_taps(s, n):
    """the oracle's linear_coord, for the transfer function's lookup"""
    u = fmaf(s, F(n), F(-0.5))
    u = np.where(~(u > F(-1)), F(-1), u).astype(F)
    u = np.where(u > F(n), F(n), u).astype(F)
    fl = np.floor(u).astype(F)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), (u - fl).astype(F)


def _clamp_first_channel(t, p, qc):
    d, h, w = t.shape
    x0, x1, fx = _clamped_cell(p[:, 0], w); y0, y1, fy = _clamped_cell(p[:, 1], h); z0, z1, fz = _clamped_cell(p[:, 2], d)
    if qc:
        fx, fy, fz = qc_weight(fx), qc_weight(fy), qc_weight(fz)
    c00 = lerpf(t[z0, y0, x0], t[z0, y0, x1], fx); c10 = lerpf(t[z0, y1, x0], t[z0, y1, x1], fx)
    c01 = lerpf(t[z1, y0, x0], t[z1, y0, x1], fx); c11 = lerpf(t[z1, y1, x0], t[z1, y1, x1], fx)
    return lerpf(lerpf(c00, c10, fy), lerpf(c01, c11, fy), fz)


def decoded_tf(oracle, tf):
    """the oracle's float4 table of an RGBA8 transfer function: sRGB-decoded rgb, alpha / 255"""
    L = oracle.lib()
    srgb = np.array([L.vpo_srgb_to_linear(c) for c in range(256)], F)
    out = np.empty(tf.shape, F)
    out[..., :3] = srgb[tf[..., :3]]
    out[..., 3] = tf[..., 3].astype(F) / F(255)
    return out


def clamp_first(oracle, case, filt):
    """the colours of the clamp-first formula at the case's points (LINEAR or quasi-cubic)"""
    assert filt in ("linear", "quasicubic")
    p, t = case.points, case.texels
    r = _clamp_first_channel(t[..., 0] if case.channels == 2 else t, p, filt == "quasicubic")
    g = _clamp_first_channel(t[..., 1], p, filt == "quasicubic") if case.channels == 2 else np.zeros_like(r)
    tf = decoded_tf(oracle, case.tf)
    x0, x1, fx = _index_clamped_taps(r, tf.shape[1]); y0, y1, fy = _index_clamped_taps(g, tf.shape[0])
    f4 = lambda f: f[:, None]
    a = lerpf(tf[y0, x0], tf[y0, x1], f4(fx)); b = lerpf(tf[y1, x0], tf[y1, x1], f4(fx))
    return lerpf(a, b, f4(fy))
