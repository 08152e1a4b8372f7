"""GPU: float volumes whose special texels (NaN, +-inf, a finite pair whose difference overflows, a pair just under the boundary atlas's
threshold) sit at CHOSEN positions relative to the sampler's clamps, brick borders and short axes — tests/float_special_cases.py, whose
conditions tests/test_float_special_cases.py proves on the oracle alone.  The sampler (probe_sample, 32-bit and wide tables, the boundary
atlas where it stays in use) and all eight renderers against the CPU oracle, bit for bit, and the two renderer lives that the life fuzz
found outside its default seeds (lao 27, lao 75: an R32F volume with one NaN and one inf texel, texel 1 of an axis beside a finite texel 0).

What these cases catch: GL clamps the tap indices of the unclamped u = s N - 0.5; a sampler that clamps u first and keeps the cell
(t[0], t[1]) at weight 0 below the first texel centre gives fma(0, t[1] - t[0], t[0]) = NaN instead of t[0] whenever t[1] - t[0] is not
finite (vpt_device.h linear_cell, below_first)."""
import types

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.scene import Node, Transform

import float_special_cases as S
import renderer_life_cases as L
from conftest import orbit_camera
from test_gpu_parity import assert_same_bits
from test_gpu_fuzz import MCM_BUFFERS
from test_gpu_renderer_life import OracleModel, RecordingRng, Replay, both_replays
from test_gpu_dos import Scene as DosScene, sweep as dos_sweep

pytestmark = pytest.mark.gpu

F = np.float32
GROUPS = {"r32f": lambda c: c.main and c.channels == 1, "rg32f": lambda c: c.main and c.channels == 2, "r32f-short": lambda c: not c.main}


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", S.FILTERS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_probe_sample_equals_the_oracle_wherever_the_special_texel_sits(gpu_ctx, oracle, group, filt):
    """every case of the group: probe_sample at the case's points = vpo_sample_volume_color, bit for bit, with 32-bit and with wide tables;
    the boundary atlas gives the bricks' samples where it stays in use (the pair under its threshold) and is refused for every other case"""
    cases = [c for c in S.cases() if GROUPS[group](c)]
    assert len(cases) >= 80
    failed = []
    for c in cases:
        want = S.expected(oracle, c, filt)
        gvol = vpt_amd.Volume.from_array(gpu_ctx, c.texels, filt)
        r = vpt_amd.MCMRenderer(gpu_ctx, gvol, orbit_camera(1.0), None, {'resolution': 16, 'transform': Transform(Node())})
        r.setTransferFunction(c.tf)
        try:
            for wide in (False, True):
                gvol.set_wide_tables(wide)
                assert_same_bits(r.probe_sample(c.points), want, "%s %s, %s tables" % (c, filt, "wide" if wide else "32-bit"))
            gvol.set_wide_tables(False)
            if c.atlas:
                assert_same_bits(r.probe_sample_boundary(c.points), r.probe_sample(c.points), "%s %s: atlas against bricks" % (c, filt))
            else:
                with pytest.raises(vpt_amd.VptError):
                    r.probe_sample_boundary(c.points)
        except AssertionError as e:
            failed.append("%s: %s" % (c, str(e).splitlines()[0]))
        finally:
            r.destroy(); gvol.destroy()
    assert not failed, "%d of %d cases differ:\n%s" % (len(failed), len(cases), "\n".join(failed))


# ---- the renderers ---------------------------------------------------------------------------------------------------------------------------
DIMS = (5, 6, 8)                                       # (nz, ny, nx)
W, H = 48, 40
RENDER_SPECIALS = ("+inf", "nan", "overflow")


def special_volume(special, axis, channels=1):
    """noise in [0.2, 0.9] with the special texel at index 1 of `axis`, in the middle of the other two axes; two channels: the special sits in
    channel axis % 2.  The overflowing pair fills a quarter of PLANES 0 and 1 of the axis (the low half of both other axes): one pair poisons
    a clamp-first sample only where its combined weight on the other two axes exceeds 0.57, a fifth of a texel's footprint — one or two
    pixels of a frame this small, or none —, and whole planes end every ray in its first step, whatever the sampler gives"""
    rng = np.random.default_rng(100 + axis)
    texels = rng.uniform(0.2, 0.9, size=DIMS + ((2,) if channels == 2 else ())).astype(F)
    view = texels[..., axis % 2] if channels == 2 else texels
    planes = np.moveaxis(view, 2 - axis, 0)            # [index along the axis][...]
    values = S.SPECIALS[special]
    if len(values) == 2:
        na, nb = planes.shape[1] // 2 + 1, planes.shape[2] // 2 + 1
        planes[0, :na, :nb], planes[1, :na, :nb] = values
    else:
        pos = [DIMS[2] // 2, DIMS[1] // 2, DIMS[0] // 2]
        pos[axis] = 1
        view[pos[2], pos[1], pos[0]] = values[0]
    return texels


def low_faces_camera():
    """at (-, -, -) of the cube's centre, looking at it: the rays enter through the faces x = 0, y = 0 and z = 0"""
    return orbit_camera(W / H, yaw=-2.4, pitch=0.6, dist=1.7)


def configure(r, kind):
    if kind == "mip":
        r.steps = 17
    elif kind == "eam":
        r.slices = 12; r.extinction = 40
    elif kind == "mcs":
        r.extinction = 5
    elif kind == "mcm":
        r.extinction = 7; r.anisotropy = 0.3; r.bounces = 3; r.steps = 3
    elif kind == "iso":
        r.steps = 20; r.isovalue = 0.5
    elif kind == "depth":
        r.slices = 24; r.extinction = 4; r.threshold = 0.5       # the threshold is crossed after several samples: each one's alpha counts
    elif kind == "lao":                                # occlusion and shadows on; 7 + 4 + 4 taps per step, five steps: tens of taps a pixel
        r.slices = 5; r.extinction = 100
        r.localAmbientOcclusion = True; r.softShadows = True
        r.numLAOSamples = 1; r.LAOStepSize = 0.3; r.numShadowSamples = 2
    elif kind == "dos":
        r.slices = 10; r.steps = 5; r.extinction = 40


def render_against_the_oracle(gpu_ctx, oracle, kind, texels, filt="linear", options=()):
    """two passes (MCM: three) of `kind`: every buffer of every pass and sample_count() against the oracle"""
    tf = S.transfer_function(2 if texels.ndim == 4 else 1)
    what = "%s %s %s" % (kind, texels.shape, filt)
    if kind == "dos":                                  # the slice sweep has its own driver
        sc = DosScene(gpu_ctx, oracle, texels, W, H, filt, tf=tf, camera=low_faces_camera())
        r = sc.renderer()
        configure(r, kind)
        try:
            dos_sweep(sc, oracle, r, 2, what)
        finally:
            r.destroy(); sc.gvol.destroy()
        return
    gvol = vpt_amd.Volume.from_array(gpu_ctx, texels, filt)
    rng = RecordingRng(1)
    r = vpt_amd.RendererFactory(kind)(gpu_ctx, gvol, low_faces_camera(), None,
                                      {'resolution': (W, H), 'transform': Transform(Node()), 'rng': rng, 'fused': False})
    try:
        for opt, val in options:
            r.set_option(opt, val)
        r.setTransferFunction(tf)
        configure(r, kind)
        model = OracleModel(oracle, kind, (W, H))
        model.scene(texels, filt, tf, None)
        Replay.lao(types.SimpleNamespace(kind=kind, r=r, model=model))
        n0 = len(rng.log)
        r.reset()
        model.reset(r._matrix(), F(rng.log[n0]) if kind == "mcm" else None)       # (MCM's reset draws its own seed)
        for k in range(3 if kind == "mcm" else 2):
            r.render()
            image = model.render_pass(r._u)
            state = model.state()
            if kind == "mcm":
                for b, s in zip(MCM_BUFFERS, state):
                    assert_same_bits(r.read(b), s, "%s: state buffer %d, pass %d" % (what, b, k))
            else:
                assert_same_bits(r.read(N.BUFFER_FRAME), state[1], "%s: frame buffer, pass %d" % (what, k))
                assert_same_bits(r.read(N.BUFFER_ACCUM), state[0], "%s: accumulation buffer, pass %d" % (what, k))
            assert_same_bits(r.getTexture().view(np.uint16), image, "%s: the image, pass %d" % (what, k))
        want = model.samples()
        assert r.sample_count() == want, "%s: sample_count() %d, the oracle %d" % (what, r.sample_count(), want)
    finally:
        r.destroy(); gvol.destroy()


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
@pytest.mark.parametrize("special", RENDER_SPECIALS)
@pytest.mark.parametrize("kind", L.KINDS + ["dos"])
def test_renderers_with_the_special_texel_at_index_1(gpu_ctx, oracle, kind, special, axis):
    render_against_the_oracle(gpu_ctx, oracle, kind, special_volume(special, axis))


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
@pytest.mark.parametrize("special", RENDER_SPECIALS)
@pytest.mark.parametrize("kind", ["mip", "mcm"])
@pytest.mark.parametrize("form", ["quasicubic", "rg32f"])
def test_the_other_filter_and_two_channels(gpu_ctx, oracle, form, kind, special, axis):
    if form == "quasicubic":
        render_against_the_oracle(gpu_ctx, oracle, kind, special_volume(special, axis), "quasicubic")
    else:
        render_against_the_oracle(gpu_ctx, oracle, kind, special_volume(special, axis, channels=2))


@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
@pytest.mark.parametrize("special", RENDER_SPECIALS)
def test_mcm_without_tile_classes(gpu_ctx, oracle, special, axis):
    render_against_the_oracle(gpu_ctx, oracle, "mcm", special_volume(special, axis), options=((N.OPTION_TILE_CLASSES, 0),))


# ---- the two lives the life fuzz left open ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [27, 75])
def test_the_lao_lives_with_a_special_texel_beside_texel_0(gpu_ctx, oracle, seed):
    """renderer_life_cases lives lao 27 (sample_count() was 1008 low) and lao 75 (one texel differed), outside the default seeds: the
    whole life and its plain twin, as tests/test_gpu_renderer_life.py replays them"""
    s = L.setup('lao', seed)
    assert any(fmt == 'R32F' and not np.isfinite(t).all() for fmt, _, t in s.volumes)
    both_replays(gpu_ctx, oracle, s)
