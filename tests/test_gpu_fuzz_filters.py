"""GPU: the randomised differential test of tests/test_gpu_fuzz.py over what it does not draw — the quasi-cubic filter in all eight
renderers, the narrow storage formats (SNORM, 16-bit normalised, packed) against the oracle's rendering of their decoded texels, float
environment maps in MCS and MCM, and the option paths of the quasi-cubic kernels.  Every comparison is bit for bit against the CPU oracle
(same_bits on every buffer of every pass, after the last pass for lazy cases); fast math stays off.  Case seeds are fixed and start at
20000; what a case adds to random_case's draws comes from a second generator.  The conditions the drawn cases must meet (the filter is
exercised, HDR values exceed 1) are asserted on the oracle alone in tests/test_oracle_filters_env.py."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.scene import Node, Transform, mvp_inverse_matrix
from vpt_amd.synthetic import GoldenRatioRng

from test_gpu_fuzz import KINDS, MCM_BUFFERS, random_case, random_camera, same_bits, run_random_scene
from test_gpu_dos import random_sweep
from test_volume_formats import snorm, decode_packed
from test_gpu_volume_formats import packed_volume, PACKED
from test_gpu_norm16 import decode as decode16, norm16_context

pytestmark = pytest.mark.gpu

# case seeds for which random_case draws a one-channel byte volume: the cases below give it its format themselves
PLAIN = [s for s in range(24000, 25000) if s % 3 != 1 and s % 5 != 2]
QC_SEEDS, DOS_SEEDS, FORMAT_SEEDS, HDR_SEEDS = 16, 12, 6, 12
# The quasi-cubic cases, by renderer: seeds of PLAIN's kind, four of each volume format (case seed % 4), chosen on the oracle alone so that
# per format three of them (DOS: two) give an image that differs from the LINEAR oracle's and one does not (a camera that misses the
# cube, a constant or a one-voxel volume) — tests/test_oracle_filters_env.py asserts the resulting condition.  Random cameras and
# parameters leave the filter without effect on the image more often than not, so a plain run of seeds would not meet it.
QC_CASES = {
    "mip": [20000, 20001, 20003, 20006, 20009, 20015, 20018, 20019, 20030, 20031, 20036, 20045, 20049, 20084, 20100, 20106],
    "eam": [20300, 20301, 20303, 20304, 20306, 20309, 20310, 20315, 20318, 20319, 20330, 20333, 20340, 20345, 20375, 20376],
    "mcs": [20600, 20601, 20603, 20606, 20610, 20616, 20619, 20628, 20630, 20639, 20645, 20646, 20649, 20651, 20661, 20688],
    "mcm": [20900, 20901, 20903, 20906, 20909, 20913, 20931, 20933, 20934, 20939, 20940, 20948, 20954, 20960, 20963, 20990],
    "iso": [21200, 21201, 21203, 21206, 21209, 21210, 21213, 21219, 21230, 21239, 21240, 21248, 21251, 21264, 21270, 21293],
    "depth": [21500, 21501, 21503, 21506, 21524, 21569, 21575, 21618, 21635, 21636, 21641, 21648, 21654, 21659, 21681, 22410],
    "lao": [21800, 21801, 21803, 21804, 21806, 21809, 21810, 21813, 21818, 21821, 21824, 21830, 21836, 21839, 21843, 21851],
    "dos": [22100, 22101, 22103, 22104, 22106, 22109, 22113, 22115, 22119, 22128, 22130, 22230],
}
assert all(len(QC_CASES[k]) == QC_SEEDS for k in KINDS) and len(QC_CASES["dos"]) == DOS_SEEDS
VOLUME_FORMATS = ("R8", "RG8", "R32F", "RG32F")
FILTERS = ("nearest", "linear", "quasicubic")


def as_format(vol, fmt, frng):
    """a byte volume [d][h][w] in one of VOLUME_FORMATS (the float forms as random_case makes them: values outside [0, 1] too)"""
    if fmt == "RG8":
        return np.ascontiguousarray(np.stack([vol, frng.integers(0, 256, size=vol.shape, dtype=np.uint8) if frng.uniform() < 0.7 else (255 - vol)], axis=-1))
    if fmt in ("R32F", "RG32F"):
        f = (vol.astype(np.float32) / np.float32(255.0) * np.float32(frng.uniform(0.5, 1.6)) + np.float32(frng.uniform(-0.3, 0.2))).astype(np.float32)
        if frng.uniform() < 0.5:
            f = f.astype(np.float16).astype(np.float32)
        if fmt == "RG32F":
            f = np.ascontiguousarray(np.stack([f, frng.uniform(-0.2, 1.3, size=f.shape).astype(np.float32)], axis=-1))
        return f
    return vol


def quasicubic_case(kind, i):
    """case i of `kind` ("dos": the eighth renderer): random_case's draws, the volume in format case seed % 4, the quasi-cubic filter"""
    case_seed = QC_CASES[kind][i]
    rng, vol, size, tf, env, _, model = random_case(case_seed)
    vol = as_format(vol, VOLUME_FORMATS[case_seed % 4], np.random.default_rng(30000 + case_seed))
    return case_seed, (rng, vol, size, tf, env, "quasicubic", model)


def float_map(kind, i, frng):
    """finite texels in [0, 64): float32, float16 or [h][w][3]; every third a 1x1 constant; some alphas below 1 for MCS"""
    h, w = (1, 1) if i % 3 == 0 else (int(frng.integers(1, 7)), int(frng.integers(1, 10)))
    form = int(frng.integers(0, 3))
    env = frng.uniform(0, 64, size=(h, w, 3 if form == 2 else 4)).astype(np.float32)
    if form != 2:
        env[..., 3] = 1.0
        if kind == "mcs":
            low = frng.uniform(size=(h, w)) < 0.5
            env[..., 3][low] = frng.uniform(0, 1, size=int(low.sum()))
    return np.ascontiguousarray(env.astype(np.float16) if form == 1 else env)


def hdr_case(kind, i):
    """case i of MCS / MCM with a float environment map; every fourth with a quasi-cubic volume"""
    case_seed = 23000 + ("mcs", "mcm").index(kind) * HDR_SEEDS + i
    rng, vol, size, tf, _, filt, model = random_case(case_seed)
    env = float_map(kind, i, np.random.default_rng(31000 + case_seed))
    return case_seed, (rng, vol, size, tf, env, "quasicubic" if i % 4 == 3 else filt, model)


# ---- quasi-cubic, all eight renderers -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(QC_SEEDS))
def test_quasicubic_random_scene(gpu_ctx, oracle, kind, i):
    case_seed, case = quasicubic_case(kind, i)
    run_random_scene(gpu_ctx, oracle, kind, case_seed, case, nthreads=4)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("i", range(DOS_SEEDS))
def test_quasicubic_dos_random_scene(gpu_ctx, oracle, i):
    case_seed, case = quasicubic_case("dos", i)
    random_sweep(gpu_ctx, oracle, case_seed, case)


# ---- storage formats against the oracle at fuzz shapes --------------------------------------------------------------------------------------
def finite_words(fmt, dims, frng):
    """packed words whose two channels decode to finite values (the float formats: exponents below their Inf / NaN codes)"""
    bits = 16 if PACKED[fmt][3] == np.uint16 else 32
    words = frng.integers(0, 1 << bits, size=dims, dtype=np.uint64).astype(PACKED[fmt][3])
    if fmt == N.FORMAT_R11F_G11F_B10F:
        words = (words & ~np.uint32((31 << 6) | (31 << 17))) | (frng.integers(0, 17, size=dims).astype(np.uint32) << 6) | \
                (frng.integers(0, 17, size=dims).astype(np.uint32) << 17)
    if fmt == N.FORMAT_RGB9_E5:
        words = (words & np.uint32(0x07FFFFFF)) | (frng.integers(0, 25, size=dims).astype(np.uint32) << 27)
    return words


def native_volume(name, dims, frng):
    """texels of `dims` (depth, height, width) in storage format `name` -> (upload(ctx, filt) -> Volume, the R32F / RG32F decoded texels)"""
    if name in ("R8_SNORM", "RG8_SNORM"):
        s = frng.integers(-128, 128, size=dims + ((2,) if name[:2] == "RG" else ()), dtype=np.int16).astype(np.int8)
        return (lambda ctx, filt: vpt_amd.Volume.from_array(ctx, s, filt, snorm=True)), np.ascontiguousarray(snorm(s))
    if name in ("R16", "RG16", "R16_SNORM", "RG16_SNORM"):
        lo, hi, dtype = (-32768, 32768, np.int16) if name.endswith("SNORM") else (0, 65536, np.uint16)
        c = frng.integers(lo, hi, size=dims + ((2,) if name[:2] == "RG" else ())).astype(dtype)
        return (lambda ctx, filt: vpt_amd.Volume.from_array(ctx, c, filt, norm16=True)), np.ascontiguousarray(decode16(c))
    fmt = getattr(N, "FORMAT_" + name)
    words = finite_words(fmt, dims, frng)
    return (lambda ctx, filt: packed_volume(ctx, words, fmt, filt)), np.ascontiguousarray(decode_packed(words, fmt))


STORAGE_FORMATS = ("R8_SNORM", "RG8_SNORM", "R16", "RG16", "R16_SNORM", "RG16_SNORM",
                   "RGB565", "RGBA4", "RGB5_A1", "RGB10_A2", "R11F_G11F_B10F", "RGB9_E5")


def format_case(name, i):
    """case i of storage format `name`: random_case's shapes, camera, tables and model; native texels of the format; kind and filter rotate"""
    k = STORAGE_FORMATS.index(name) * FORMAT_SEEDS + i
    case_seed = PLAIN[k]
    rng, vol, size, tf, env, _, model = random_case(case_seed)
    upload, decoded = native_volume(name, vol.shape, np.random.default_rng(32000 + case_seed))
    assert np.isfinite(decoded).all()
    return case_seed, KINDS[k % len(KINDS)], upload, (rng, decoded, size, tf, env, FILTERS[(k // len(KINDS) + i) % 3], model)


@pytest.fixture(scope="module")
def norm16_ctx():
    ctx = norm16_context()
    yield ctx
    ctx.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", STORAGE_FORMATS)
@pytest.mark.parametrize("i", range(FORMAT_SEEDS))
def test_storage_format_random_scene(gpu_ctx, request, oracle, name, i):
    case_seed, kind, upload, case = format_case(name, i)
    ctx = request.getfixturevalue("norm16_ctx") if name.endswith("16_SNORM") else gpu_ctx
    run_random_scene(ctx, oracle, kind, case_seed, case, upload=upload, nthreads=4)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,dims", [("R8_SNORM", (2, 3, 4096)), ("R16_SNORM", (4096, 2, 3)), ("RG16", (3, 4096, 1)), ("RGB565", (1, 1, 4096))])
def test_storage_formats_at_extreme_volume_shapes(gpu_ctx, oracle, name, dims):
    """texels of 1, 2, 4 and 8 bytes (packed words are stored decoded, as RG32F) along a 4096-voxel axis next to 1..3-voxel axes: the
    per-size brick and apron arithmetic and the wide offset tables at their edge (tests/test_gpu_fuzz.py: test_extreme_volume_shapes)"""
    upload, decoded = native_volume(name, dims, np.random.default_rng(sum(dims) + len(name)))
    w, h = 90, 70
    camera = random_camera(np.random.default_rng(11), w / h)
    model = Transform(Node())
    m = mvp_inverse_matrix(camera, model)
    for filt in FILTERS:
        osc = oracle.OracleScene(decoded, filt)
        gvol = upload(gpu_ctx, filt)
        r = vpt_amd.EAMRenderer(gpu_ctx, gvol, camera, None, {'resolution': (w, h), 'transform': model, 'rng': GoldenRatioRng()})
        r.slices = 200
        o = oracle.OracleRenderer('eam', osc, w, h)
        r.reset(); o.reset(oracle.make_frame(w, h, m))
        r.render()
        o.render(oracle.make_frame(w, h, m, offset=np.float32(GoldenRatioRng()()), steps=200, extinction=100, mix=1.0, nthreads=4))
        same_bits(r.read(N.BUFFER_ACCUM), o.acc, "eam %s volume %s %s accumulation" % (name, dims, filt))
        same_bits(r.getTexture().view(np.uint16), o.out, "eam %s volume %s %s" % (name, dims, filt))
        assert r.sample_count() == o.samples
        r.destroy(); gvol.destroy()


# ---- HDR environment maps -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", ["mcs", "mcm"])
@pytest.mark.parametrize("i", range(HDR_SEEDS))
def test_float_environment_map_random_scene(gpu_ctx, oracle, kind, i):
    case_seed, case = hdr_case(kind, i)
    assert np.isfinite(case[4].astype(np.float32)).all()
    run_random_scene(gpu_ctx, oracle, kind, case_seed, case, nthreads=4)


# ---- the option paths of the quasi-cubic kernels, once each ----------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["mcm", "eam"])
def test_quasicubic_option_paths_against_the_oracle(gpu_ctx, oracle, kind):
    """the MISS-tile check, the general pass, wide tables, fused and eager frame sequences: six passes each, every buffer against the oracle"""
    rng = np.random.default_rng(78)
    vol = rng.integers(0, 256, size=(18, 20, 22), dtype=np.uint8)
    tf = rng.integers(0, 256, size=(1, 16, 4), dtype=np.uint8)
    w, h, passes = 88, 60, 6
    camera = random_camera(np.random.default_rng(9), w / h)
    model = Transform(Node())
    gvol = vpt_amd.Volume.from_array(gpu_ctx, vol, "quasicubic")

    def make(options=()):
        r = vpt_amd.RendererFactory(kind)(gpu_ctx, gvol, camera, None, {'resolution': (w, h), 'transform': model, 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf)
        for opt, val in options:
            r.set_option(opt, val)
        r.extinction = 7 if kind == "mcm" else 40
        r.reset()
        return r

    # the oracle, driven by the uniforms of a plain render() loop
    o = oracle.OracleRenderer(kind, oracle.OracleScene(vol, "quasicubic", tf=tf), w, h)
    m = mvp_inverse_matrix(camera, model)
    o.reset(oracle.make_frame(w, h, m, seed=np.float32(GoldenRatioRng()())) if kind == "mcm" else oracle.make_frame(w, h, m))
    ref = make()
    for _ in range(passes):
        ref.render()
        u = ref._u
        fr = oracle.make_frame(w, h, np.array(list(u.mvp_inverse), np.float32), nthreads=4)
        fr.seed = u.rand_seed; fr.offset = u.offset; fr.step = u.step_size; fr.extinction = u.extinction; fr.anisotropy = u.anisotropy
        fr.max_bounces = u.max_bounces; fr.steps = u.steps; fr.mix = u.mix; fr.blur = u.blur
        o.render(fr)

    def hold(r, what):
        if kind == "mcm":
            for b, s in zip(MCM_BUFFERS, o.state):
                same_bits(r.read(b), s, "%s quasi-cubic, %s: state %d" % (kind, what, b))
        else:
            same_bits(r.read(N.BUFFER_ACCUM), o.acc, "%s quasi-cubic, %s: accumulation" % (kind, what))
        same_bits(r.getTexture().view(np.uint16), o.out, "%s quasi-cubic, %s: render" % (kind, what))
        r.destroy()

    hold(ref, "render()")
    if kind == "mcm":                                  # (the MISS-tile check is an MCM option)
        r = make(((N.OPTION_VERIFY_TILE_CLASSES, 1),))
        for _ in range(passes):
            r.render()
        assert r.tile_classes()[2] == 0, r.tile_classes()
        hold(r, "tile classes verified")
    r = make(((N.OPTION_TILE_CLASSES, 0),))
    for _ in range(passes):
        r.render()
    hold(r, "no tile classes")
    gvol.set_wide_tables(True)
    r = make()
    for _ in range(passes):
        r.render()
    hold(r, "wide tables")
    gvol.set_wide_tables(False)
    r = make(); r.play(passes, fused=True); hold(r, "play fused")
    r = make(); r.play(passes, use_graph=False); hold(r, "play eager")
    gvol.destroy()
