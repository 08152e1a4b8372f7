"""The quasi-cubic sampler contract in fp32 numpy (the LINEAR cell and taps, the weights f' = (f * f) * (3 - 2 f),
the format's lerp order with fmaf from libm), and the bounds that hold a renderer to the reference's shader text with that filter
(tests/golden/quasicubic_r05.json).  One statement of each, shared by the GPU tests (tests/test_gpu_quasicubic.py) and the CPU oracle's
(tests/test_oracle_filters_env.py)."""
import base64
import ctypes
import ctypes.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "quasicubic_r05.json")))
F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]
fmaf = np.vectorize(lambda a, b, c: _libm.fmaf(a, b, c), otypes=[np.float32])


def lerpf(a, b, f):
    return fmaf(f, (b - a).astype(F), a)


def qc_weight(f):
    f = np.asarray(f, F)
    return ((f * f).astype(F) * (F(3) - (F(2) * f).astype(F))).astype(F)


def cell(s, n):
    """linear_cell: u = med3(fma(s, n, -0.5), 0, n - 1) (NaN -> 0), i = trunc(u), f = fract(u); then the quasi-cubic weight"""
    u = fmaf(s.astype(F), F(n), F(-0.5))
    u = np.where(np.isnan(u), F(0), np.clip(u, F(0), F(n - 1))).astype(F)
    i = u.astype(np.int64)
    return i, qc_weight((u - np.floor(u)).astype(F))


def qc_sample(texels, p):
    """texture(uVolume, p) of one channel under VPT_FILTER_QUASI_CUBIC: texels [d][h][w] float32 (taps as the format's path holds them),
    normalised afterwards by the caller (UNSIGNED_BYTE: * fl32(1/255))"""
    d, h, w = texels.shape
    x0, fx = cell(p[:, 0], w); y0, fy = cell(p[:, 1], h); z0, fz = cell(p[:, 2], d)
    x1, y1, z1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1), np.minimum(z0 + 1, d - 1)
    t = lambda z, y, x: texels[z, y, x].astype(F)
    c00 = lerpf(t(z0, y0, x0), t(z0, y0, x1), fx); c10 = lerpf(t(z0, y1, x0), t(z0, y1, x1), fx)
    c01 = lerpf(t(z1, y0, x0), t(z1, y0, x1), fx); c11 = lerpf(t(z1, y1, x0), t(z1, y1, x1), fx)
    return lerpf(lerpf(c00, c10, fy), lerpf(c01, c11, fy), fz)


def tf_alpha_1d(r, width):
    """sample_tf's alpha for a transfer function whose alpha bytes are 0 .. width - 1 (fl32(c / 255)) and whose rgb is 0"""
    t = (np.arange(width, dtype=F) / F(255)).astype(F)
    dt = (t[np.minimum(np.arange(width) + 1, width - 1)] - t).astype(F)
    u = fmaf(r.astype(F), F(width), F(-0.5))
    u = np.where(np.isnan(u), F(0), np.clip(u, F(0), F(width - 1))).astype(F)
    i = u.astype(np.int64)
    return fmaf((u - np.floor(u)).astype(F), dt[i], t[i])


def tf_alpha_2d(r, g, alpha):
    """sample_tf2d's alpha (linear_taps in x then y, lerp4) for an alpha table alpha[h][w] (bytes)"""
    h, w = alpha.shape
    t = (alpha.astype(F) / F(255)).astype(F)

    def taps(s, n):
        u = fmaf(s.astype(F), F(n), F(-0.5))
        u = np.where(~(u > F(-1)), F(-1), u).astype(F)
        u = np.where(u > F(n), F(n), u).astype(F)
        fl = np.floor(u).astype(F)
        i = fl.astype(np.int64)
        return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), (u - fl).astype(F)
    x0, x1, fx = taps(r, w); y0, y1, fy = taps(g, h)
    return lerpf(lerpf(t[y0, x0], t[y0, x1], fx), lerpf(t[y1, x0], t[y1, x1], fx), fy)


def probe_points(dims, rng, n=10000):
    d, h, w = dims
    rand = rng.uniform(-0.2, 1.2, size=(n, 3)).astype(F)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    centres = np.stack([(x + 0.5) / w, (y + 0.5) / h, (z + 0.5) / d], axis=-1).reshape(-1, 3).astype(F)
    # cell borders of the LINEAR cell: u = s N - 0.5 integral at texel centres; the texture's own borders s = k / N
    borders = np.stack([rng.integers(0, w + 1, n // 4) / w, rng.integers(0, h + 1, n // 4) / h, rng.integers(0, d + 1, n // 4) / d], axis=1).astype(F)
    specials = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 0.5], F)
    edge = np.array(np.meshgrid(specials, specials, specials, indexing="ij"), F).reshape(3, -1).T
    return np.concatenate([rand, centres, borders, edge]).astype(F)


def bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d differ, first %s: got %r want %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])


# ---- the renderers against the reference's shader text with the quasi-cubic sampler -------------------------------------------------------
def arr(b64, dtype, shape):
    return np.frombuffer(base64.b64decode(b64), dtype=dtype).reshape(shape).copy()


def close(got, want, rel, abs_, what, max_outliers=0):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(np.abs(got - want) <= abs_ + rel * np.abs(want))
    bad &= ~(np.isnan(got) & np.isnan(want))
    n = int(bad.reshape(bad.shape[0] * bad.shape[1], -1).any(axis=1).sum())
    assert n <= max_outliers, "%s: %d pixels differ (allowed %d); worst |d| = %g" % (what, n, max_outliers, float(np.nanmax(np.abs(got - want) * bad)))


def fixture_scene(scene):
    """scene "r8" or "rg8_inside" -> (scene record, renderer records, volume, transfer function, environment map, inverse MVP)"""
    s, R = FX["scene_" + scene], FX["renderers_" + scene]
    vol = arr(s["volume_u8"], np.uint8, s["volume_shape"]); tf = arr(s["tf_rgba8"], np.uint8, s["tf_shape"]); env = arr(s["env_rgba8"], np.uint8, s["env_shape"])
    return s, R, vol, tf, env, arr(s["mvp_inverse_f32"], np.float32, (16,))


class ReferenceTextBounds:
    """what a renderer's buffers must keep to the fixture after each sequence's last frame (the bounds tests/test_glsl_reference.py holds the
    CPU oracle to on the LINEAR fixture of the same program); `who` names the implementation in the messages"""

    def __init__(self, scene, who):
        s, self.R = FX["scene_" + scene], FX["renderers_" + scene]
        self.W, self.H, self.who = s["width"], s["height"], who

    def mip(self, acc_u8):
        """MIP: the R8 accumulator, byte for byte"""
        H, W = self.H, self.W
        assert (np.asarray(acc_u8).reshape(H, W) == arr(self.R["mip"]["acc_u8"], np.uint8, (H, W))).all(), "%s: MIP accumulator" % self.who

    def eam(self, acc_u8):
        """EAM: the RGBA8 accumulator, byte for byte"""
        H, W = self.H, self.W
        assert (np.asarray(acc_u8).reshape(H, W, 4) == arr(self.R["eam"]["acc_u8"], np.uint8, (H, W, 4))).all(), "%s: EAM accumulator" % self.who

    def iso(self, acc_f16, image_f16):
        """ISO: the closest hit in half floats within one half ulp, the shaded image within the oracle's bounds"""
        H, W, fx = self.H, self.W, self.R["iso"]
        close(np.asarray(acc_f16).reshape(H, W, 4).astype(np.float32), arr(fx["acc_f16"], np.float16, (H, W, 4)).astype(np.float32),
              1e-3, 1e-3, "%s: ISO closest hit" % self.who, max_outliers=1)
        close(np.asarray(image_f16).reshape(H, W, 4).astype(np.float32), arr(fx["image_f16"], np.float16, (H, W, 4)).astype(np.float32),
              2e-2, 4e-3, "%s: ISO shaded image" % self.who, max_outliers=2)

    def depth(self, acc_f32):
        H, W = self.H, self.W
        close(np.asarray(acc_f32).reshape(H, W, 1), arr(self.R["depth"]["acc_f32"], np.float32, (H, W, 1)), 1e-5, 1e-6,
              "%s: Depth accumulator" % self.who, max_outliers=1)

    def mcm(self, state_f32):
        """MCM: the same photon histories (position, direction + bounces, transmittance, radiance + paths ended)"""
        H, W = self.H, self.W
        for q in range(4):
            got, want = np.asarray(state_f32[q]).reshape(H, W, 4), arr(self.R["mcm"]["state_f32"][q], np.float32, (H, W, 4))
            assert (np.abs(got.astype(np.float64) - want) <= 1e-4 + (2e-3 if q == 0 else 5e-4) * np.abs(want.astype(np.float64))).all(), \
                "%s: MCM buffer %d" % (self.who, q)
            if q in (1, 3):                                  # bounces, paths ended: exact
                assert (got[..., 3] == want[..., 3]).all(), "%s: MCM buffer %d counts" % (self.who, q)
