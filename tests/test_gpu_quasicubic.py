"""GPU: the quasi-cubic volume filter (VPT_FILTER_QUASI_CUBIC, sampler variant VPT_V_QCUBIC = 256).

The probes are held bit for bit to an fp32 numpy restatement of the sampler contract (the LINEAR cell and taps, the
weights f' = (f * f) * (3 - 2 f), the format's lerp order with fmaf from libm); the renderers to what the reference's shader text computes
with that filter (tests/golden/quasicubic_r05.json) and to themselves across the tile classes, the general pass and the frame sequences."""
import os
import sys

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.scene import Transform, Node, default_camera
from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng

from quasicubic_contract import (F, qc_sample, tf_alpha_1d, tf_alpha_2d, probe_points, bits_equal,     # the numpy contract, shared with the
                                 fixture_scene, ReferenceTextBounds)                                   # CPU oracle's tests
from test_volume_formats import snorm, decode_packed
from test_gpu_volume_formats import packed_volume, same, CLASSES, BUFFERS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (13, 17, 11)                      # depth, height, width: odd, not a multiple of the 4^3 bricks


def alpha_ramp_tf(width=256):
    tf = np.zeros((1, width, 4), np.uint8)
    tf[0, :, 3] = np.arange(width)
    return tf


def probe_renderer(ctx, vol):
    return vpt_amd.MIPRenderer(ctx, vol, default_camera(1.0), None, {'resolution': (8, 8)})


# each case: (name, make volume (ctx) -> Volume, channel texels [(taps, normalise)])
def format_cases():
    rng = np.random.default_rng(11)
    u8 = sphere_volume(0, noise=60.0, dims=DIMS)
    u8_2 = np.stack([u8, rng.integers(0, 256, size=DIMS, dtype=np.uint8)], axis=-1)
    f32 = rng.uniform(0, 1, size=DIMS).astype(F)
    f32_2 = rng.uniform(0, 1, size=DIMS + (2,)).astype(F)
    s8 = rng.integers(-128, 128, size=DIMS, dtype=np.int16).astype(np.int8)
    s8_2 = rng.integers(-128, 128, size=DIMS + (2,), dtype=np.int16).astype(np.int8)
    words = rng.integers(0, 1 << 16, size=DIMS, dtype=np.uint64).astype(np.uint16)
    inv = F(0.00392156862745098)
    return [
        ("R8", lambda c: vpt_amd.Volume.from_array(c, u8, 'quasicubic'), [(u8.astype(F), inv)]),
        ("RG8", lambda c: vpt_amd.Volume.from_array(c, u8_2, 'quasicubic'), [(u8_2[..., 0].astype(F), inv), (u8_2[..., 1].astype(F), inv)]),
        ("R32F", lambda c: vpt_amd.Volume.from_array(c, f32, 'quasicubic'), [(f32, None)]),
        ("RG32F", lambda c: vpt_amd.Volume.from_array(c, f32_2, 'quasicubic'), [(f32_2[..., 0], None), (f32_2[..., 1], None)]),
        ("R8_SNORM", lambda c: vpt_amd.Volume.from_array(c, s8, 'quasicubic', snorm=True), [(snorm(s8), None)]),
        ("RG8_SNORM", lambda c: vpt_amd.Volume.from_array(c, s8_2, 'quasicubic', snorm=True), [(snorm(s8_2[..., 0]), None), (snorm(s8_2[..., 1]), None)]),
        ("RGB565", lambda c: packed_volume(c, words, N.FORMAT_RGB565, 'quasicubic'),
         [(decode_packed(words, N.FORMAT_RGB565)[..., 0], None), (decode_packed(words, N.FORMAT_RGB565)[..., 1], None)]),
    ]


@pytest.mark.timeout(600)
def test_probes_equal_the_numpy_contract_bit_for_bit(gpu_ctx):
    """every format under the quasi-cubic filter: the sample (through the transfer function's alpha) of >= 10^4 points each"""
    rng = np.random.default_rng(7)
    p = probe_points(DIMS, rng)
    assert p.shape[0] >= 10000
    for name, make, chans in format_cases():
        v = make(gpu_ctx)
        r = probe_renderer(gpu_ctx, v)
        vals = []
        for texels, norm in chans:
            s = qc_sample(texels, p)
            vals.append((s * norm).astype(F) if norm is not None else s)
        if len(chans) == 1:
            r.setTransferFunction(alpha_ramp_tf())
            bits_equal(r.probe_sample(p)[:, 3], tf_alpha_1d(vals[0], 256), "%s quasi-cubic probes" % name)
        else:
            for k in range(2):                    # the 2-D lookup once along r, once along g
                alpha = np.zeros((256, 256), np.uint8)
                alpha[:] = np.arange(256)[None, :] if k == 0 else np.arange(256)[:, None]
                tf = np.zeros((256, 256, 4), np.uint8); tf[..., 3] = alpha
                r.setTransferFunction(tf)
                bits_equal(r.probe_sample(p)[:, 3], tf_alpha_2d(vals[0], vals[1], alpha), "%s quasi-cubic probes, channel %d" % (name, k))
        r.destroy(); v.destroy()


@pytest.mark.timeout(300)
def test_boundary_atlas_equals_the_bricks_on_the_faces(gpu_ctx):
    rng = np.random.default_rng(8)
    p = rng.uniform(-0.3, 1.3, size=(30000, 3)).astype(F)
    p[:5000, 0] = rng.choice(np.array([-0.25, 1.25, -1e-7, 1 + 1e-7, np.inf, -np.inf], F), 5000)
    p = p[((p > 1) | (p < 0)).any(axis=1)]
    for name, make, chans in format_cases():
        v = make(gpu_ctx)
        r = probe_renderer(gpu_ctx, v)
        r.setTransferFunction(colour_tf(64, 1 if len(chans) == 1 else 48))
        bits_equal(r.probe_sample_boundary(p), r.probe_sample(p), "%s atlas = bricks" % name)
        r.destroy(); v.destroy()


@pytest.mark.timeout(120)
def test_quasicubic_differs_from_linear_on_noise_and_not_on_a_constant(gpu_ctx):
    rng = np.random.default_rng(9)
    p = rng.uniform(0, 1, size=(20000, 3)).astype(F)
    tf = colour_tf(256)
    for vol, differs in ((sphere_volume(0, noise=60.0, dims=DIMS), True), (np.full(DIMS, 137, np.uint8), False)):
        out = {}
        for filt in ('linear', 'quasicubic'):
            v = vpt_amd.Volume.from_array(gpu_ctx, vol, filt)
            r = probe_renderer(gpu_ctx, v)
            r.setTransferFunction(tf)
            out[filt] = r.probe_sample(p)
            r.destroy(); v.destroy()
        ndiff = int((out['linear'].view(np.uint32) != out['quasicubic'].view(np.uint32)).any(axis=1).sum())
        if differs:
            assert ndiff > p.shape[0] // 4, ndiff            # (the sphere's empty corners sample 0 under either filter)
        else:
            assert ndiff == 0, ndiff


# ---- the renderers against the reference's shader text with the quasi-cubic sampler -------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("scene", ["r8", "rg8_inside"])
def test_hip_against_the_reference_text(gpu_ctx, scene):
    """MIP, EAM, ISO, Depth (and MCM, on the R8 scene) of libvpt_hip.so on the fixture's scenes after each sequence's last frame, within the bounds
    tests/test_glsl_reference.py holds the CPU oracle to on the LINEAR fixture of the same program"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_glsl_fixtures as M
    s, R, vol, tf, env, m = fixture_scene(scene)
    W, H = s["width"], s["height"]
    bounds = ReferenceTextBounds(scene, "libvpt_hip.so")     # (the comparisons themselves: shared with the CPU oracle's test)
    gvol = vpt_amd.Volume.from_array(gpu_ctx, vol, s["filter"])

    def run(kind, seeds, attrs, cls=None, per_frame=None):
        it = iter(seeds)
        r = (cls or vpt_amd.RendererFactory(kind))(gpu_ctx, gvol, M.camera_node(W / H, *s["camera"]), env,
                                                   {'resolution': (W, H), 'transform': vpt_amd.Transform(vpt_amd.Node()), 'rng': lambda: next(it)})
        r.setTransferFunction(tf)
        for k, v in attrs.items():
            setattr(r, k, v)
        r.reset()
        for u in R[kind]["uniforms_per_frame"]:
            if per_frame:
                per_frame(r, u)
            r.render()
            assert (np.array(list(r._u.mvp_inverse), np.float32).view(np.uint32) == m.view(np.uint32)).all()
        return r
    offsets = lambda kind: [u["offset"] for u in R[kind]["uniforms_per_frame"]]
    u0 = lambda kind: R[kind]["uniforms_per_frame"][0]
    # MIP and EAM: the R8 / RGBA8 accumulator, byte for byte
    r = run('mip', offsets('mip'), {'steps': round(1.0 / u0('mip')["step"])})
    bounds.mip(r.read(N.BUFFER_ACCUM))
    r.destroy()
    r = run('eam', offsets('eam'), {'slices': round(1.0 / u0('eam')["step"]), 'extinction': u0('eam')["extinction"]})
    bounds.eam(r.read(N.BUFFER_ACCUM))
    r.destroy()
    # ISO: the closest hit in half floats within one half ulp, the shaded image within the oracle's bounds

    class FixtureISO(vpt_amd.ISORenderer):               # the fixture's light direction and gradient step, as uploaded
        def _prepare_render(self):
            for i in range(3):
                self._u.light_direction[i] = float(u0('iso')["light"][i])
            self._u.gradient_step = float(np.float32(u0('iso')["gradient_step"]))
            return self._u
    r = run('iso', offsets('iso'), {'steps': u0('iso')["steps"], 'isovalue': u0('iso')["isovalue"]}, FixtureISO)
    bounds.iso(r.read(N.BUFFER_ACCUM), r.getTexture())
    r.destroy()
    # Depth
    d0 = u0('depth')
    r = run('depth', offsets('depth'), {'slices': round(1.0 / d0["step"]), 'extinction': d0["extinction"], 'threshold': d0["threshold"], 'random': True})
    bounds.depth(r.read(N.BUFFER_ACCUM))
    r.destroy()
    if "mcm" not in R:
        gvol.destroy()
        return
    # MCM: the same photon histories
    c0 = u0('mcm')
    r = run('mcm', [s["mcm_reset_seed"]] + [u["seed"] for u in R['mcm']["uniforms_per_frame"]],
            {'extinction': c0["extinction"], 'bounces': c0["max_bounces"], 'steps': c0["steps"]},
            per_frame=lambda r, u: setattr(r, 'anisotropy', u["anisotropy"]))
    bounds.mcm([r.read(b) for b in (N.BUFFER_MCM_POSITION, N.BUFFER_MCM_DIRECTION, N.BUFFER_MCM_TRANSMITTANCE, N.BUFFER_MCM_RADIANCE)])
    r.destroy(); gvol.destroy()


# ---- the renderers against themselves ------------------------------------------------------------------------------------------------------
def render(ctx, gvol, kind, w=61, h=47, tf=None, options=(), play=None, passes=2, extinction=40):
    """reset + `passes` render() (or play(*play)) -> every buffer, getTexture() last"""
    r = CLASSES[kind](ctx, gvol, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    if tf is not None:
        r.setTransferFunction(tf)
    for opt, val in options:
        r.set_option(opt, val)
    if kind == 'mcm':
        r.extinction = extinction
    r.reset()
    if play is not None:
        r.play(*play[0], **play[1])
    else:
        for _ in range(passes):
            r.render()
    out = [r.read(b) for b in BUFFERS.get(kind, [N.BUFFER_RENDER, N.BUFFER_FRAME, N.BUFFER_ACCUM])] + [r.getTexture()]
    classes = r.tile_classes() if kind == 'mcm' else None
    r.destroy()
    return out, classes


@pytest.mark.timeout(600)
def test_mcm_1080p_tile_classes_equal_the_general_pass(gpu_ctx):
    """R8, default options: the HIT tiles through the quasi-cubic general kernel from a tile list, the MISS tiles through the LINEAR
    MISS-tile kernel; 8 frames equal the general pass bit for bit, with the MISS-tile check and with fast math"""
    vol = sphere_volume(0, noise=40.0, dims=(45, 38, 51))
    v = vpt_amd.Volume.from_array(gpu_ctx, vol, 'quasicubic')
    tf = colour_tf(256)
    for extra in ((), ((N.OPTION_VERIFY_TILE_CLASSES, 1),), ((N.OPTION_FAST_MATH, 1),)):
        a, cls = render(gpu_ctx, v, 'mcm', 1920, 1080, tf=tf, options=extra, passes=8)
        hit, miss, violations = cls
        assert hit > 0 and miss > 0, cls
        assert violations == 0, cls
        b, _ = render(gpu_ctx, v, 'mcm', 1920, 1080, tf=tf, options=extra + ((N.OPTION_TILE_CLASSES, 0),), passes=8)
        same(a, b, "1080p classes against the general pass %s" % (extra,))
    v.destroy()


@pytest.mark.timeout(600)
def test_play_equals_repeated_render(gpu_ctx):
    tf = colour_tf(256)
    vol = sphere_volume(0, noise=40.0, dims=DIMS)
    v = vpt_amd.Volume.from_array(gpu_ctx, vol, 'quasicubic')
    v2 = vpt_amd.Volume.from_array(gpu_ctx, np.stack([vol, vol[::-1]], axis=-1), 'quasicubic')
    for gv, t, what in ((v, tf, 'R8'), (v2, colour_tf(64, 48), 'RG8')):
        for kind in ('mip', 'eam', 'mcs', 'mcm'):
            want, _ = render(gpu_ctx, gv, kind, tf=t, passes=8)      # (8 passes: MCM plays fewer eagerly where the tile classes are in force)
            same(render(gpu_ctx, gv, kind, tf=t, play=((8,), {'use_graph': False}))[0], want, '%s %s play eager' % (what, kind))
            same(render(gpu_ctx, gv, kind, tf=t, play=((8,), {'fused': True}))[0], want, '%s %s play fused' % (what, kind))
            if kind == 'mcm':
                same(render(gpu_ctx, gv, kind, tf=t, play=((8,), {'frames': True}))[0], want, '%s mcm play frames' % what)
                o = ((N.OPTION_FAST_MATH, 1),)
                same(render(gpu_ctx, gv, kind, tf=t, options=o, play=((8,), {'fused': True}))[0],
                     render(gpu_ctx, gv, kind, tf=t, options=o, passes=8)[0], '%s mcm fast math play fused' % what)
    v.destroy(); v2.destroy()


@pytest.mark.timeout(300)
def test_lao_and_dos_run_deterministic_and_differ_from_linear(gpu_ctx):
    tf = colour_tf(256)
    vol = sphere_volume(0, noise=60.0, dims=DIMS)
    vq = vpt_amd.Volume.from_array(gpu_ctx, vol, 'quasicubic')
    vl = vpt_amd.Volume.from_array(gpu_ctx, vol, 'linear')
    for kind in ('lao', 'dos'):
        a, _ = render(gpu_ctx, vq, kind, tf=tf)
        b, _ = render(gpu_ctx, vq, kind, tf=tf)
        same(a, b, '%s quasi-cubic twice' % kind)
        c, _ = render(gpu_ctx, vl, kind, tf=tf)
        assert np.ascontiguousarray(a[-1]).tobytes() != np.ascontiguousarray(c[-1]).tobytes(), '%s: quasi-cubic image equals LINEAR' % kind
    vq.destroy(); vl.destroy()


@pytest.mark.timeout(300)
def test_set_filter_switches_the_next_frame_without_a_reload(gpu_ctx):
    tf = colour_tf(256)
    vol = sphere_volume(0, noise=60.0, dims=DIMS)
    v = vpt_amd.Volume.from_array(gpu_ctx, vol, 'linear')
    ref = {f: vpt_amd.Volume.from_array(gpu_ctx, vol, f) for f in ('linear', 'quasicubic')}
    for kind in ('eam', 'mcm'):
        want = {f: render(gpu_ctx, ref[f], kind, tf=tf)[0] for f in ref}
        r = CLASSES[kind](gpu_ctx, v, default_camera(61 / 47), None, {'resolution': (61, 47), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf)
        if kind == 'mcm':
            r.extinction = 40
        for f in ('linear', 'quasicubic', 'linear', 'quasicubic'):
            v.setFilter(f)
            r.rng = GoldenRatioRng()                           # (the reference renders start their seeds afresh)
            r.reset()
            for _ in range(2):
                r.render()
            got = [r.read(b) for b in BUFFERS.get(kind, [N.BUFFER_RENDER, N.BUFFER_FRAME, N.BUFFER_ACCUM])] + [r.getTexture()]
            same(got, want[f], '%s after setFilter(%r)' % (kind, f))
        r.destroy()
    v.destroy()
    for x in ref.values():
        x.destroy()
