"""CPU: the oracle's quasi-cubic filter (vpo_scene.filter == 2) and float environment table (vpo_scene.env_f32), which carry the GPU's
0-ulp parity for those features (tests/test_gpu_fuzz_filters.py) — the sampler against the fp32 numpy contract bit for bit, the filter's
identities in every renderer, a float map against the RGBA8 map of the same table, the renderers against the reference's shader text
within the bounds the HIP library is held to, and the conditions the GPU file's drawn cases must meet, checked on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

from vpt_amd.scene import Node, Transform
from vpt_amd.hdr import HDRImage

from quasicubic_contract import F, qc_sample, tf_alpha_2d, probe_points, bits_equal, fixture_scene, ReferenceTextBounds
from test_gpu_fuzz import KINDS, oracle_only, run_random_scene
from test_gpu_dos import random_sweep
from test_gpu_fuzz_filters import QC_SEEDS, DOS_SEEDS, HDR_SEEDS, quasicubic_case, hdr_case

SHAPES = [(13, 17, 11), (1, 1, 1), (1, 5, 7), (3, 1, 17), (4, 4, 4), (5, 4, 9)]      # depth, height, width
INV255 = F(0.00392156862745098)


# ---- 1. the sampler against the contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", SHAPES)
def test_quasicubic_sampler_equals_the_numpy_contract_bit_for_bit(oracle, dims):
    """vpo_sample_volume (R8, R32F) and vpo_sample_volume_color (RG8, RG32F through a 2-D transfer function's alpha) at texel centres, cell
    borders, zeros, infinities, NaN and >= 10^4 random points"""
    rng = np.random.default_rng(sum(dims))
    p = probe_points(dims, rng)
    assert p.shape[0] >= 10000
    L = oracle.lib()
    xyz = [[float(v) for v in q] for q in p]
    for texels, norm in ((rng.integers(0, 256, size=dims, dtype=np.uint8), INV255), (rng.uniform(-0.3, 1.4, size=dims).astype(F), None)):
        sc = oracle.OracleScene(texels, "quasicubic")
        got = np.array([L.vpo_sample_volume(C.byref(sc.c), *q) for q in xyz], F)
        want = qc_sample(texels.astype(F), p)
        bits_equal(got, (want * norm).astype(F) if norm is not None else want, "%s %s quasi-cubic sample" % (dims, texels.dtype))
        assert oracle.OracleScene(texels, "linear").c.filter == 1 and oracle.OracleScene(texels, "nearest").c.filter == 0 and sc.c.filter == 2
    alpha = rng.integers(0, 256, size=(5, 7), dtype=np.uint8)
    tf = np.zeros((5, 7, 4), np.uint8); tf[..., 3] = alpha
    out = np.zeros(4, F)
    for texels, norm in ((rng.integers(0, 256, size=dims + (2,), dtype=np.uint8), INV255), (rng.uniform(-0.3, 1.4, size=dims + (2,)).astype(F), None)):
        sc = oracle.OracleScene(texels, "quasicubic", tf=tf)
        got = np.empty(len(xyz), F)
        for k, q in enumerate(xyz):
            L.vpo_sample_volume_color(C.byref(sc.c), *q, out.ctypes.data_as(C.c_void_p))
            got[k] = out[3]
        r, g = [qc_sample(texels[..., c].astype(F), p) for c in range(2)]
        if norm is not None:
            r, g = (r * norm).astype(F), (g * norm).astype(F)
        bits_equal(got, tf_alpha_2d(r, g, alpha), "%s %s quasi-cubic sample through the 2-D transfer function" % (dims, texels.dtype))


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------------
def buffers(o):
    if o.kind == "mcm":
        return o.state + [o.out]
    if o.kind == "dos":
        return [o.color[o.cur], o.occlusion[o.cur], o.out]
    return [o.frame, o.acc, o.out]


def oracle_run(oracle, kind, vol, filt, env=None, size=(40, 30), seed=0, draws=12):
    """the oracle's side of a scene through the fuzz drivers (camera and renderer parameters drawn from generator `draws`): three passes
    (DOS: three sweeps), every buffer"""
    rng = np.random.default_rng(draws)
    tf = np.random.default_rng(13).integers(0, 256, size=(3, 16, 4), dtype=np.uint8)
    case = (rng, vol, size, tf, env, filt, Transform(Node()))
    with oracle_only() as ctx:
        o = random_sweep(ctx, oracle, seed, case, compare=False) if kind == "dos" else run_random_scene(None, oracle, kind, seed, case, nthreads=4)
    return [b.copy() for b in buffers(o)]


def identical(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("kind", KINDS + ["dos"])
def test_quasicubic_equals_linear_where_it_must_and_differs_on_noise(oracle, kind):
    noise = np.random.default_rng(3).integers(0, 256, size=(7, 9, 11), dtype=np.uint8)
    differ = 0
    for draws in range(12, 18):                       # six cameras and parameter sets: the identities hold in each of them
        for vol in (np.full((7, 9, 11), 137, np.uint8), np.array([[[91]]], np.uint8), np.full((5, 6, 7, 2), 0.37, np.float32)):
            assert identical(oracle_run(oracle, kind, vol, "quasicubic", draws=draws), oracle_run(oracle, kind, vol, "linear", draws=draws)), \
                "%s: constant %s volume, draws %d" % (kind, vol.shape, draws)
        differ += not identical(oracle_run(oracle, kind, noise, "quasicubic", draws=draws), oracle_run(oracle, kind, noise, "linear", draws=draws))
    # (some of the six miss the cube, draw no extinction or a threshold never reached: those images cannot depend on the filter)
    assert differ >= 1, "%s: quasi-cubic equals LINEAR on noise in all six scenes" % kind


# ---- 3. a float map against the RGBA8 map of the same table -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mcs", "mcm"])
def test_float_table_of_an_rgba8_map_renders_identically(oracle, kind):
    rng = np.random.default_rng(21)
    vol = rng.integers(0, 256, size=(9, 8, 7), dtype=np.uint8)
    for shape in ((4, 7, 4), (1, 1, 4)):
        rgba8 = rng.integers(0, 256, size=shape, dtype=np.uint8)
        table = (rgba8.astype(F) / F(255)).astype(F)                       # from_unorm8 of each byte
        want = oracle_run(oracle, kind, vol, "linear", env=rgba8)
        assert identical(oracle_run(oracle, kind, vol, "linear", env=table), want), "%s: RGBA32F table of an RGBA8 map %s" % (kind, shape)
        assert not identical(oracle_run(oracle, kind, vol, "linear", env=(table * F(3)).astype(F)), want), "%s: the float table is not read" % kind


def test_oracle_scene_takes_what_the_renderers_take_for_an_environment_map(oracle):
    rng = np.random.default_rng(22)
    vol = np.zeros((2, 2, 2), np.uint8)
    rgba = rng.uniform(0, 70000, size=(3, 5, 4)).astype(F)
    assert oracle.OracleScene(vol, env=rgba).env_f32.tobytes() == rgba.tobytes()
    half = rng.uniform(0, 64, size=(3, 5, 4)).astype(np.float16)
    assert oracle.OracleScene(vol, env=half).env_f32.tobytes() == half.astype(F).tobytes()          # half widens exactly
    rgb = rng.uniform(0, 9, size=(2, 3, 3)).astype(F)
    t = oracle.OracleScene(vol, env=rgb).env_f32
    assert t.shape == (2, 3, 4) and t[..., :3].tobytes() == rgb.tobytes() and (t[..., 3] == 1).all()
    rgbe = np.array([[[128, 64, 255, 129], [200, 100, 50, 0], [1, 0, 0, 1], [255, 255, 255, 255]]], np.uint8)
    t = oracle.OracleScene(vol, env=HDRImage(rgbe, 4, 1)).env_f32              # m * 2^(e - 136), e == 0 black, alpha 1 (include/vpt.h)
    want = np.array([[[1.0, 0.5, 255 / 128, 1], [0, 0, 0, 1], [2.0 ** -135, 0, 0, 1], [255 * 2.0 ** 119] * 3 + [1]]], F)
    assert t.tobytes() == want.tobytes()
    sc = oracle.OracleScene(vol, env=rng.integers(0, 256, size=(2, 2, 4), dtype=np.uint8))
    assert sc.env_f32 is None and not sc.c.env_f32 and not oracle.OracleScene(vol).c.env_f32       # RGBA8 and no map: as before
    out = np.zeros(4, F)
    sc = oracle.OracleScene(vol, env=rgba[:1, :1])
    oracle.lib().vpo_sample_environment(C.byref(sc.c), 0.0, 1.0, 0.0, out.ctypes.data_as(C.c_void_p))
    assert out.tobytes() == rgba[0, 0].tobytes()                                # the 1x1 shortcut returns the float texel


# ---- 4. the oracle against the reference's shader text ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["r8", "rg8_inside"])
def test_oracle_against_the_reference_text(oracle, scene):
    """the comparisons, bounds and outlier allowances of tests/test_gpu_quasicubic.py's test_hip_against_the_reference_text"""
    s, R, vol, tf, env, m = fixture_scene(scene)
    W, H = s["width"], s["height"]
    bounds = ReferenceTextBounds(scene, "the oracle")
    sc = oracle.OracleScene(vol, s["filter"], tf=tf, env=env)
    assert sc.c.filter == 2

    def run(kind, frames, reset=None):
        o = oracle.OracleRenderer(kind, sc, W, H)
        o.reset(reset or oracle.make_frame(W, H, m))
        for fr in frames:
            o.render(fr)
        return o
    U = lambda kind: R[kind]["uniforms_per_frame"]
    bounds.mip(run("mip", [oracle.make_frame(W, H, m, offset=u["offset"], steps=round(1.0 / u["step"])) for u in U("mip")]).acc)
    bounds.eam(run("eam", [oracle.make_frame(W, H, m, offset=u["offset"], steps=round(1.0 / u["step"]), extinction=u["extinction"], mix=u["mix"])
                           for u in U("eam")]).acc)
    o = run("iso", [oracle.make_frame(W, H, m, offset=u["offset"], steps=u["steps"], mcm_steps=u["steps"], isovalue=u["isovalue"], light_dir=u["light"],
                                      gradient_step=u["gradient_step"]) for u in U("iso")])
    bounds.iso(o.acc.view(np.float16), o.out.view(np.float16))
    bounds.depth(run("depth", [oracle.make_frame(W, H, m, offset=u["offset"], steps=round(1.0 / u["step"]), extinction=u["extinction"],
                                                 threshold=u["threshold"], mix=u["mix"]) for u in U("depth")]).acc)
    if "mcm" in R:
        o = run("mcm", [oracle.make_frame(W, H, m, seed=u["seed"], extinction=u["extinction"], anisotropy=u["anisotropy"], max_bounces=u["max_bounces"],
                                          mcm_steps=u["steps"]) for u in U("mcm")], reset=oracle.make_frame(W, H, m, seed=s["mcm_reset_seed"]))
        bounds.mcm(o.state)


# ---- 5. the conditions on the GPU file's drawn cases, on the oracle alone -------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ["dos"])
def test_at_least_half_of_the_quasicubic_cases_exercise_the_filter(oracle, kind):
    """the oracle's image of a drawn quasi-cubic case differs from its LINEAR image in at least half the cases of every renderer (a camera
    that misses the cube, or a constant volume, legitimately gives equality)"""
    n = DOS_SEEDS if kind == "dos" else QC_SEEDS
    differ = 0
    for i in range(n):
        images = []
        for filt in ("quasicubic", "linear"):
            case_seed, case = quasicubic_case(kind, i)
            assert np.isfinite(case[1].astype(np.float32)).all()
            case = case[:5] + (filt,) + case[6:]
            with oracle_only() as ctx:
                o = random_sweep(ctx, oracle, case_seed, case, compare=False) if kind == "dos" else run_random_scene(None, oracle, kind, case_seed, case, nthreads=4)
            images.append(o.out.tobytes())
        differ += images[0] != images[1]
    assert 2 * differ >= n, "%s: %d of %d quasi-cubic cases differ from LINEAR" % (kind, differ, n)


@pytest.mark.parametrize("kind", ["mcs", "mcm"])
def test_at_least_half_of_the_float_map_cases_hold_values_above_one(oracle, kind):
    """the MCS accumulator / MCM radiance of a drawn float-map case holds a value above 1 in at least half the cases: a clamp would show"""
    above = 0
    for i in range(HDR_SEEDS):
        case_seed, case = hdr_case(kind, i)
        env = np.asarray(case[4])
        assert env.dtype in (np.float32, np.float16) and np.isfinite(env.astype(F)).all() and (env >= 0).all() and (env.astype(F) < 64).all()
        assert (i % 3 != 0 or env.shape[:2] == (1, 1)) and (i % 4 != 3 or case[5] == "quasicubic")
        with oracle_only():
            o = run_random_scene(None, oracle, kind, case_seed, case, nthreads=4)
        values = o.acc.reshape(-1, 4)[:, :3] if kind == "mcs" else o.state[3].reshape(-1, 4)[:, :3]
        above += bool((values > 1).any())
    assert 2 * above >= HDR_SEEDS, "%s: %d of %d float-map cases hold a value above 1" % (kind, above, HDR_SEEDS)
