"""GPU: HDR environment maps (vpt_renderer_set_environment_texels, include/vpt.h).  The device decode is exact in every format (read back
through vpt_probe_environment_texels); a map renders bit-identical in MCS and MCM whichever format carried its texels; HDR values reach the
photon state and the accumulators unclamped; a map switched between fused sequences is ordered after the passes that read the old one."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.hdr import HDRImage, read_hdr
from vpt_amd.scene import default_camera
from vpt_amd.synthetic import colour_tf

from conftest import orbit_camera
from test_gpu_parity import Scene, env_map, assert_same_bits, MCM_BUFFERS
from test_hdr_host import encode_hdr, rgbe_image

pytestmark = pytest.mark.gpu


def bare_renderer(gpu_ctx, kind='mcm'):
    return vpt_amd.RendererFactory(kind)(gpu_ctx, None, default_camera(1.0), None, {'resolution': (16, 16)})


def decode_rgbe(data):
    """numpy's statement of the RGBE rule: m 2^(e - 136), e = 0 black, alpha 1"""
    e = data[..., 3].astype(np.int32)
    out = np.ones(data.shape, np.float32)
    out[..., :3] = np.ldexp(data[..., :3].astype(np.float32), (e - 136)[..., None])
    out[..., :3][e == 0] = 0.0
    return out


# ---- 1. the decode ------------------------------------------------------------------------------------------------------------------
def test_every_half_pattern_decodes_exactly(gpu_ctx):
    r = bare_renderer(gpu_ctx)
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(128, 128, 4)
    r.setEnvironmentMap(halves.view(np.float16))
    got = r.environment_texels()
    want = halves.view(np.float16).astype(np.float32)
    assert_same_bits(got, want, "RGBA16F decode")               # (payloads of NaNs included: numpy keeps them)
    assert np.isnan(got).sum() == np.isnan(want).sum() == 2 * 1023
    assert (got.view(np.uint32) == 0x33800000).sum() == 1      # (the smallest subnormal half, 2^-24)
    r.destroy()


def test_every_rgbe_mantissa_and_exponent_decodes_exactly(gpu_ctx):
    r = bare_renderer(gpu_ctx)
    e, m = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    rgbe = np.stack([m, (m + 85) % 256, (m + 170) % 256, e], axis=-1).astype(np.uint8)    # row e, column m: every (m, e) in each channel
    r.setEnvironmentMap(HDRImage(rgbe, 256, 256))
    got = r.environment_texels()
    want = decode_rgbe(rgbe)
    assert_same_bits(got, want, "RGBE8 decode")
    assert (got[0, :, :3] == 0).all() and (got[..., 3] == 1).all()
    assert got[1, 1, 0] == np.float32(2.0 ** -135) and got[255, 255, 0] == np.float32(255 * 2.0 ** 119)
    r.destroy()


def test_float_texels_pass_through_and_rgba8_matches_the_old_entry(gpu_ctx):
    r = bare_renderer(gpu_ctx)
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff, 0x00400000, 0x7fc00001, 0xffbfffff,
                         0x3f800000, 0xbf800000, 0x7f7fffff, 0xff7fffff, 0x00800000], np.uint32)
    rng = np.random.default_rng(4)
    bits = np.concatenate([specials, rng.integers(0, 2 ** 32, size=4 * 37 * 5 - specials.size, dtype=np.uint64).astype(np.uint32)])
    tex = bits.view(np.float32).reshape(5, 37, 4)
    r.setEnvironmentMap(tex)
    assert_same_bits(r.environment_texels(), tex, "RGBA32F pass-through")
    # RGBA8 through the new entry == vpt_renderer_set_environment, every byte value in every channel
    rgba8 = np.stack([np.arange(256), np.arange(256)[::-1], (np.arange(256) * 7) % 256, (np.arange(256) * 3) % 256], -1).astype(np.uint8).reshape(8, 32, 4)
    r.setEnvironmentMap(rgba8)
    old = r.environment_texels()
    N.check(N.lib().vpt_renderer_set_environment_texels(r._h, rgba8.ctypes.data_as(C.c_void_p), 32, 8, N.ENV_RGBA8))
    assert_same_bits(r.environment_texels(), old, "RGBA8 through the new entry")
    assert_same_bits(old, rgba8.astype(np.float32) / np.float32(255), "RGBA8 c / 255")
    # float [h][w][3]: alpha 1 added on the host
    rgb = rng.uniform(0, 9, size=(3, 5, 3)).astype(np.float32)
    r.setEnvironmentMap(rgb)
    want = np.concatenate([rgb, np.ones((3, 5, 1), np.float32)], -1)
    assert_same_bits(r.environment_texels(), want, "RGB32F + alpha 1")
    r.setEnvironmentMap(rgb.astype(np.float16))
    assert_same_bits(r.environment_texels(), want.astype(np.float16).astype(np.float32), "RGB16F + alpha 1")
    r.destroy()


# ---- 2. - 5. rendering ----------------------------------------------------------------------------------------------------------------
def make(sc, kind, env, general=False):
    r = sc.renderer(kind)
    if env is not None:
        r.setEnvironmentMap(env)
    if kind == 'mcs':
        r.extinction = 9
    if general:
        r.set_option(N.OPTION_TILE_CLASSES, 0); r.set_option(N.OPTION_SPLIT_STREAMS, 1)
    r.reset()
    return r


def buffers(r, kind):
    if kind == 'mcm':
        return [r.read(b).copy() for b in MCM_BUFFERS] + [r.getTexture().copy()]
    return [r.read(b).copy() for b in (N.BUFFER_ACCUM, N.BUFFER_FRAME)] + [r.getTexture().copy()]


def run(sc, kind, env, mode, general=False, passes=5):
    r = make(sc, kind, env, general)
    if mode == 'render':
        for _ in range(passes):
            r.render()
    elif mode == 'eager':
        r.play(2, use_graph=False); r.play(passes - 2, use_graph=False)
    else:
        r.play(2, fused=True); r.play(passes - 2, fused=True)
    out = buffers(r, kind) + [r.sample_count()]
    r.destroy()
    return out


def same_outputs(a, b, what):
    for k, (x, y) in enumerate(zip(a[:-1], b[:-1])):
        assert_same_bits(x, y, "%s buffer %d" % (what, k))
    assert a[-1] == b[-1], what


@pytest.fixture(scope="module")
def hd(gpu_ctx, oracle):
    sc = Scene(gpu_ctx, oracle, 32, 1920, 1080, tf=colour_tf(64, 1))
    yield sc
    sc.gvol.destroy()


@pytest.mark.parametrize("kind", ["mcs", "mcm"])
@pytest.mark.parametrize("general,mode", [(False, 'render'), (False, 'eager'), (False, 'fused'), (True, 'render'), (True, 'fused')])
def test_rgba32f_table_renders_as_the_rgba8_map(gpu_ctx, hd, kind, general, mode):
    """the RGBA8 map's own decoded table (read back, not recomputed) uploaded as RGBA32F: every buffer bit-identical"""
    rgba8 = env_map(48, 24, seed=11)
    probe = bare_renderer(gpu_ctx)
    probe.setEnvironmentMap(rgba8)
    table = probe.environment_texels()
    probe.destroy()
    same_outputs(run(hd, kind, table, mode, general), run(hd, kind, rgba8, mode, general), "%s %s general=%s" % (kind, mode, general))


def hdr_table(h, w, seed):
    """an opaque float map in [0.5, 6): scaled by 16 or 1/16 it stays exact"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.5, 6.0, size=(h, w, 4)).astype(np.float32)
    t[..., 3] = 1.0
    return t


def normal_or_zero(a):
    a = np.abs(np.asarray(a, np.float32))
    return bool(((a == 0) | (a >= np.float32(2.0 ** -122))).all() and np.isfinite(a).all())


@pytest.mark.parametrize("general", [True, False])
@pytest.mark.parametrize("kind", ["mcm", "mcs"])
@pytest.mark.parametrize("scale", [16.0, 1.0 / 16.0])
def test_hdr_values_reach_the_image_unclamped(gpu_ctx, hd, scale, kind, general):
    """a power-of-two scale of an opaque map scales MCS's accumulators exactly (every operation on the map's values is homogeneous in them).
    MCM's photons start from radiance 1 (MCMRenderer.glsl:268, resetPhoton), so a pixel's first deposit is 1 + (rad - 1), rounded at the
    scale of 1 whatever the map's scale: its radiance follows the scale to within that rounding, 2^-22 of max(1, |radiance|)"""
    base = hdr_table(32, 64, seed=3)
    scaled = base.copy(); scaled[..., :3] *= np.float32(scale)
    buf = N.BUFFER_MCM_RADIANCE if kind == "mcm" else N.BUFFER_ACCUM
    outs = []
    for t in (base, scaled):
        r = make(hd, kind, t, general)
        for _ in range(4):
            r.render()
        outs.append(r.read(buf).copy())
        r.destroy()
    want, got = outs
    assert normal_or_zero(want), "%s: the unscaled buffer holds subnormals (the scaling would not be exact)" % kind
    assert want[..., :3].max() > 1.0, kind
    assert_same_bits(got[..., 3], want[..., 3], "%s alpha" % kind)
    if kind == "mcm":
        w = want[..., :3].astype(np.float64) * scale
        d = np.abs(got[..., :3] - w) / np.maximum(1.0, np.abs(w))
        assert d.max() <= 2.0 ** -22, "%s x %g: %g" % (kind, scale, d.max())
        assert (got[..., :3] != w).mean() < 0.1, kind                # (most of it scales exactly)
    else:
        assert_same_bits(got[..., :3], want[..., :3] * np.float32(scale), "%s x %g" % (kind, scale))


def test_constant_hdr_map_reaches_miss_pixels_exactly(gpu_ctx, hd):
    c = np.array([[[3.5, 0.25, 12.0, 1.0]]], np.float32)
    rad = {}
    for name, env in (("white", None), ("hdr", c)):
        r = make(hd, 'mcm', env)
        for _ in range(3):
            r.render()
        rad[name] = r.read(N.BUFFER_MCM_RADIANCE).copy()
        r.destroy()
    escaped = (rad["white"][..., :3] == 1.0).all(-1)               # every photon left with transmittance 1: the cube's MISS pixels
    assert escaped.sum() > hd.w * hd.h // 4
    assert_same_bits(rad["hdr"][escaped][:, :3], np.broadcast_to(c[0, 0, :3], (int(escaped.sum()), 3)), "MCM MISS pixels")


def test_rgbe_file_and_half_map_render_as_their_float_tables(gpu_ctx, hd, tmp_path):
    img = rgbe_image(24, 48, seed=8)
    img[..., 3] = 126 + img[..., 3] % 12                            # values around 2^-10 .. 2^2 (a sky, not random exponents)
    img[0, :5, 3] = 0                                               # (and black texels)
    path = tmp_path / "sky.hdr"
    path.write_bytes(encode_hdr(img, extra=(b"EXPOSURE=1.0",)))
    hdr = read_hdr(str(path))
    assert hdr.data.tobytes() == img.tobytes()
    half = (np.random.default_rng(2).uniform(0, 8, size=(16, 32, 4))).astype(np.float16)
    half[..., 3] = 1.0
    half[0, 0, :3] = np.array([1, 2, 3], np.uint16).view(np.float16)  # (subnormal halves)
    for kind in ("mcs", "mcm"):
        same_outputs(run(hd, kind, hdr, 'fused'), run(hd, kind, decode_rgbe(img), 'fused'), "%s RGBE8 file" % kind)
        same_outputs(run(hd, kind, half, 'render'), run(hd, kind, half.astype(np.float32), 'render'), "%s RGBA16F" % kind)


@pytest.mark.parametrize("size", [(8, 16), (40, 80)])
@pytest.mark.parametrize("kind", ["mcs", "mcm"])
def test_switching_maps_between_fused_sequences(gpu_ctx, hd, kind, size):
    """size (8, 16): the table of the RGBA8 map is overwritten in stream order; (40, 80): a new table replaces it"""
    rgba8, table = env_map(16, 8, seed=1), hdr_table(*size, seed=5)

    def seq(sync):
        r = make(hd, kind, rgba8)
        r.play(4, fused=True)
        if sync:
            gpu_ctx.synchronize()
        r.setEnvironmentMap(table)
        r.play(4, fused=True)
        out = buffers(r, kind)
        r.destroy()
        return out

    a, b = seq(False), seq(True)
    for k, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, "%s switch buffer %d" % (kind, k))


def test_mcs_marcher_classes_follow_an_opaque_map_switched_to_a_translucent_one(gpu_ctx, oracle):
    """the fixed point of the MISS pixels needs an opaque map: after the switch to alpha < 1 the classes must give the general pass's buffers"""
    sc = Scene(gpu_ctx, oracle, 24, 208, 144, tf=colour_tf(48, 1), camera=orbit_camera(208 / 144, 0.7, -0.3, 3.2))
    opaque, translucent = hdr_table(8, 16, seed=6), hdr_table(8, 16, seed=7)
    translucent[..., 3] = 0.375

    def seq(classes):
        r = sc.renderer('mcs')
        r.setEnvironmentMap(opaque)
        r.set_option(N.OPTION_TILE_CLASSES, classes)
        r.reset()
        for _ in range(3):
            r.render()
        r.setEnvironmentMap(translucent)
        r.reset()
        for _ in range(4):
            r.render()
        r.play(3, fused=True)
        out = [r.read(N.BUFFER_ACCUM).copy(), r.getTexture().copy(), r.sample_count()]
        r.destroy()
        return out

    same_outputs(seq(1), seq(0), "MCS classes after the switch")
    sc.gvol.destroy()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    r = bare_renderer(gpu_ctx)
    L = N.lib()
    px = np.ones((2, 2, 4), np.float32)
    p = px.ctypes.data_as(C.c_void_p)
    for fmt in (-1, 4, 99):
        assert L.vpt_renderer_set_environment_texels(r._h, p, 1, 1, fmt) == N.ERR_INVALID
        assert b"unknown environment format" in L.vpt_last_error()
    for w, h in ((0, 1), (1, 0), (16385, 1), (1, 16385)):
        assert L.vpt_renderer_set_environment_texels(r._h, p, w, h, N.ENV_RGBA32F) == N.ERR_INVALID
        assert b"out of range" in L.vpt_last_error()
    assert L.vpt_renderer_set_environment_texels(r._h, None, 1, 1, N.ENV_RGBA32F) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    small = np.empty(3 * 4, np.float32)
    r.setEnvironmentMap(px)
    assert L.vpt_probe_environment_texels(r._h, small.ctypes.data_as(C.c_void_p), 3) == N.ERR_INVALID
    with pytest.raises(TypeError):
        r.setEnvironmentMap(np.ones((2, 2, 4), np.float64))
    assert_same_bits(r.environment_texels(), px, "the map survives refused calls")     # (nothing refused touched it)
    r.destroy()
