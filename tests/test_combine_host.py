"""CPU: the numpy statement of the two-volume operations (vpt_amd.combine_texels, vpt_amd.compare_stats) held to loops over Python integers
and to the identities the contract implies, the plain-JS twin (js/vpt/combine.js, through js/test/test_combine_host.js) held to the numpy
statement, the `combine` option of RenderingContext, and the C symbols without a device."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.combine import OPS, STATS, check_channel, check_op, check_weights, combine_texels, compare_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 1), (7, 5, 1), (23, 19, 21))                      # nx, ny, nz
NOISE = (23, 19, 21)
DTYPES = (np.uint8, np.uint16)
ONE_WIDTH_OPS = ('min', 'max', 'absdiff', 'pair')


def blends(M):
    """the ten (wa, wb, offset) of the contract's table and its extremes; entries 6 and 7 are the extreme ones"""
    return ((256, 256, 0), (256, -256, 0), (256, -256, (M + 1) // 2), (128, 128, 0), (512, -256, 0), (-256, 0, M), (4096, 4096, -M), (-4096, -4096, M),
            (77, 151, 3), (0, 256, 0))


EXTREME = (6, 7)


def value_sets(dtype, shape, seed):
    """[(name, a, b)], [nz][ny][nx] texels: uniform noise over every code; heavy ties from {0, 1, M - 1, M}; (uint16) the codes that tell
    whole-code unsigned arithmetic from byte-wise or signed"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    M = int(np.iinfo(dtype).max)
    draw = lambda codes: np.array(codes, dtype)[rng.integers(0, len(codes), size=(nz, ny, nx))]
    sets = [('noise', rng.integers(0, M + 1, size=(nz, ny, nx)).astype(dtype), rng.integers(0, M + 1, size=(nz, ny, nx)).astype(dtype)),
            ('ties', draw([0, 1, M - 1, M]), draw([0, 1, M - 1, M]))]
    if dtype == np.uint16:
        codes = [0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFF00]
        sets.append(('bytes', draw(codes), draw(codes)))
    return sets


def loop(a, b, op, lo=0, hi=0, fill=0, wa=0, wb=0, offset=0):
    """the contract over Python integers, voxel by voxel"""
    M = int(np.iinfo(a.dtype).max)
    A, B = [int(v) for v in a.reshape(-1)], [int(v) for v in b.reshape(-1)]
    if op == 'pair':
        return np.array([[x, y] for x, y in zip(A, B)], a.dtype).reshape(a.shape + (2,))
    one = {'mask': lambda x, y: x if lo <= y <= hi else fill, 'min': min, 'max': max, 'absdiff': lambda x, y: abs(x - y),
           'blend': lambda x, y: min(max(((wa * x + wb * y + 128) >> 8) + offset, 0), M)}[op]
    return np.array([one(x, y) for x, y in zip(A, B)], a.dtype).reshape(a.shape)


def mask_range(dtype_b):
    Mb = int(np.iinfo(dtype_b).max)
    return Mb // 4, Mb - Mb // 4


def test_the_rounding_of_the_shift():
    """>> 8 after + 128 is floor(x / 256 + 1 / 2): -0.5 -> 0, -1.5 -> -1, the average of 1 and 2 is 2; numpy's and Python's shifts agree"""
    for x, want in ((-128, 0), (-384, -1), (128 * 1 + 128 * 2, 2), (-129, -1), (127, 0), (128, 1)):
        assert (x + 128) >> 8 == want and int((np.int64(x) + 128) >> 8) == want
    assert 4096 * 65535 * 2 + 128 == 536862848 < 2 ** 31
    one, two = np.array([[[1]]], np.uint8), np.array([[[2]]], np.uint8)
    assert combine_texels(one, two, 'blend', wa=128, wb=128).item() == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_equals_loops_over_python_integers(dtype):
    M = int(np.iinfo(dtype).max)
    for n, shape in enumerate(SHAPES):
        for name, a, b in value_sets(dtype, shape, seed=5 + n):
            what = "%s %s %s" % (np.dtype(dtype).name, shape, name)
            for op in ONE_WIDTH_OPS:
                assert combine_texels(a, b, op).tobytes() == loop(a, b, op).tobytes(), (op, what)
            for wa, wb, offset in blends(M):
                assert combine_texels(a, b, 'blend', wa=wa, wb=wb, offset=offset).tobytes() == loop(a, b, 'blend', wa=wa, wb=wb, offset=offset).tobytes(), (wa, wb, offset, what)
            for other in DTYPES:                                  # a mask of either width
                m = (b.astype(np.uint32) * (257 if other == np.uint16 and dtype == np.uint8 else 1) >> (8 if other == np.uint8 and dtype == np.uint16 else 0)).astype(other)
                lo, hi = mask_range(other)
                want = loop(a, m, 'mask', lo=lo, hi=hi, fill=M - 1)
                assert combine_texels(a, m, 'mask', lo=lo, hi=hi, fill=M - 1).tobytes() == want.tobytes(), (np.dtype(other).name, what)
            two = np.stack([a, b], axis=-1)                       # a two-channel second volume
            assert combine_texels(a, two, 'absdiff', channel=1).tobytes() == loop(a, b, 'absdiff').tobytes()
            assert combine_texels(b, two, 'absdiff', channel=0).tobytes() == loop(b, a, 'absdiff').tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_identities(dtype):
    M = int(np.iinfo(dtype).max)
    for name, a, b in value_sets(dtype, NOISE, seed=5):
        wide_a, wide_b = a.astype(np.int64), b.astype(np.int64)
        blend = lambda wa, wb, offset=0, x=a, y=b: combine_texels(x, y, 'blend', wa=wa, wb=wb, offset=offset)
        assert (combine_texels(a, b, 'absdiff') == combine_texels(a, b, 'max') - combine_texels(a, b, 'min')).all()
        assert blend(256, 0).tobytes() == a.tobytes()
        assert blend(0, 256).tobytes() == b.tobytes()
        assert blend(-256, 0, M, x=blend(-256, 0, M)).tobytes() == a.tobytes()          # inversion twice
        assert (blend(256, 256) == np.minimum(wide_a + wide_b, M)).all()
        assert (blend(256, -256) == np.maximum(wide_a - wide_b, 0)).all()
        assert (blend(128, 128) == (wide_a + wide_b + 1) >> 1).all()
        assert combine_texels(a, b, 'mask', lo=0, hi=M).tobytes() == a.tobytes()
        assert combine_texels(a, b, 'mask').tobytes() == a.tobytes()                    # hi None: b's largest code
        pair = combine_texels(a, b, 'pair')
        assert pair.shape == a.shape + (2,) and pair.dtype == a.dtype
        assert pair[..., 0].tobytes() == a.tobytes() and pair[..., 1].tobytes() == b.tobytes()
        assert combine_texels(a, a, 'absdiff').max() == 0 and combine_texels(a, a, 'min').tobytes() == a.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_blend_cases_are_not_degenerate(dtype):
    """a result cannot pass by copying a source, by being constant or by clamping everything"""
    M = int(np.iinfo(dtype).max)
    _, a, b = value_sets(dtype, NOISE, seed=5)[0]
    lively = 0
    for k, (wa, wb, offset) in enumerate(blends(M)):
        raw = ((wa * a.astype(np.int64) + wb * b.astype(np.int64) + 128) >> 8) + offset
        clamped = float(((raw < 0) | (raw > M)).mean())
        out = combine_texels(a, b, 'blend', wa=wa, wb=wb, offset=offset)
        distinct = len(np.unique(out))
        assert distinct > 1, (wa, wb, offset)
        if (wa, wb, offset) != (0, 256, 0):
            assert out.tobytes() != b.tobytes(), (wa, wb, offset)
        assert out.tobytes() != a.tobytes(), (wa, wb, offset)
        if k in EXTREME:
            assert 0.0 < clamped < 1.0, (wa, wb, offset, clamped)
        elif clamped < 0.6 and distinct > 200:
            lively += 1
    assert lively >= 6, lively


def test_mixed_widths_are_for_the_mask_alone_and_bad_arguments_raise():
    a8, a16 = np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.uint16)
    for op in ONE_WIDTH_OPS + ('blend',):
        with pytest.raises(ValueError, match="one width"):
            combine_texels(a8, a16, op)
    assert combine_texels(a8, a16, 'mask', lo=0, hi=65535).shape == a8.shape
    for bad in ('mean', 0, None):
        with pytest.raises(ValueError, match="combine op is"):
            check_op(bad)
    assert [check_op(name) for name in ('mask', 'min', 'max', 'absdiff', 'blend', 'pair')] == [0, 1, 2, 3, 4, 5] and len(OPS) == 6
    for wa, wb, offset in ((4097, 0, 0), (0, -4097, 0), (1.5, 0, 0), (True, 0, 0), (0, 0, 65536), (0, 0, -65536), (0, 0, None)):
        with pytest.raises(ValueError, match="blend (weight|offset)"):
            check_weights(wa, wb, offset)
    assert check_weights(-4096, 4096, -65535) == (-4096, 4096, -65535)
    assert check_channel(0, 1) == 0 and check_channel(1, 2) == 1
    for channel, channels in ((1, 1), (2, 2), (-1, 2), (True, 2), ('0', 2)):
        with pytest.raises(ValueError, match="channel"):
            check_channel(channel, channels)
    for kwargs in ({'lo': 3, 'hi': 2}, {'hi': 256}, {'fill': 256}, {'lo': -1}, {'fill': 1.0}):
        with pytest.raises(ValueError, match="mask"):
            combine_texels(a8, a8, 'mask', **kwargs)
    with pytest.raises(ValueError, match="size"):
        combine_texels(a8, np.zeros((2, 3, 5), np.uint8), 'min')
    with pytest.raises(ValueError):
        combine_texels(np.zeros((2, 3, 4), np.float32), a8, 'min')
    with pytest.raises(ValueError):
        combine_texels(np.zeros((2, 3, 4, 2), np.uint8), a8, 'min')


def stats_loop(a, b, a_range, b_range):
    A, B = [int(v) for v in a.reshape(-1)], [int(v) for v in b.reshape(-1)]
    ia = [a_range[0] <= x <= a_range[1] for x in A]
    ib = [b_range[0] <= y <= b_range[1] for y in B]
    d = [abs(x - y) for x, y in zip(A, B)]
    return {'voxels': len(A), 'differing': sum(1 for v in d if v), 'max_abs': max(d), 'sum_abs': sum(d), 'sum_sq': sum(v * v for v in d),
            'in_a': sum(ia), 'in_b': sum(ib), 'both': sum(1 for p, q in zip(ia, ib) if p and q)}


def test_compare_stats_equal_python_integer_sums():
    for dtype_a in DTYPES:
        for dtype_b in DTYPES:                                    # mixed widths are taken
            for n, shape in enumerate(SHAPES):
                for name, a, _ in value_sets(dtype_a, shape, seed=11 + n):
                    b = value_sets(dtype_b, shape, seed=17 + n)[0 if name == 'noise' else 1][2]
                    ra, rb = mask_range(dtype_a), mask_range(dtype_b)
                    got = compare_stats(a, b, ra, rb)
                    want = stats_loop(a, b, ra, rb)
                    assert {k: got[k] for k in STATS} == want, (np.dtype(dtype_a).name, np.dtype(dtype_b).name, shape, name)
                    assert all(type(got[k]) is int for k in STATS)
                    peak = max(int(np.iinfo(dtype_a).max), int(np.iinfo(dtype_b).max))
                    if want['in_a'] + want['in_b']:
                        assert got['dice'] == 2 * want['both'] / (want['in_a'] + want['in_b'])
                        assert got['jaccard'] == want['both'] / (want['in_a'] + want['in_b'] - want['both'])
                    assert got['mse'] == want['sum_sq'] / want['voxels']
                    if want['sum_sq']:
                        assert got['psnr'] == 10.0 * math.log10(peak * peak / got['mse'])


def test_compare_stats_of_identical_and_of_empty_ranges():
    _, a, _ = value_sets(np.uint16, NOISE, seed=19)[0]
    same = compare_stats(a, a)
    assert [same[k] for k in STATS] == [a.size, 0, 0, 0, 0, a.size, a.size, a.size]
    assert same['dice'] == 1.0 and same['jaccard'] == 1.0 and same['mse'] == 0.0 and same['psnr'] is None
    zero = np.zeros((3, 4, 5), np.uint8)
    none = compare_stats(zero, zero, (1, 255), (1, 255))
    assert none['in_a'] == none['in_b'] == none['both'] == 0 and none['dice'] is None and none['jaccard'] is None
    two = np.stack([zero, zero + 7], axis=-1)
    assert compare_stats(zero, two, channel=1)['sum_abs'] == 7 * zero.size and compare_stats(zero, two, channel=0)['sum_abs'] == 0
    for bad in ((3, 2), (0,), 'ab', (0.0, 1.0), (-1, 4)):
        with pytest.raises(ValueError, match="a_range"):
            compare_stats(zero, zero, bad)


# ---- the package, the ABI, the option --------------------------------------------------------------------------------------------
def test_the_package_exports_the_statement():
    for name in ('combine_texels', 'compare_stats', 'OPS', 'check_op', 'check_weights', 'check_channel'):
        assert name in vpt_amd.__all__ and getattr(vpt_amd, name) is getattr(vpt_amd.combine, name)
    for name in ('combine', 'combine_timed', 'mask', 'minimum', 'maximum', 'absdiff', 'blend', 'pair', 'compare'):
        assert callable(getattr(vpt_amd.Volume, name))


def test_symbols_exist_and_null_arguments_are_refused_without_a_device():
    L = N.lib()
    for name in ("vpt_volume_combine", "vpt_volume_combine_timed", "vpt_volume_compare"):
        assert name in N.SYMBOLS and hasattr(L, name)
    p, out, ms, counts = N.CombineParams(), C.c_void_p(), C.c_double(), (C.c_uint64 * 8)()
    assert L.vpt_volume_combine(None, None, C.byref(p), C.byref(out)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_combine_timed(None, None, C.byref(p), C.byref(out), C.byref(ms)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_compare(None, None, 0, 0, 255, 0, 255, counts) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert C.sizeof(N.CombineParams) == 32
    assert (N.COMBINE_MASK, N.COMBINE_MIN, N.COMBINE_MAX, N.COMBINE_ABSDIFF, N.COMBINE_BLEND, N.COMBINE_PAIR) == (0, 1, 2, 3, 4, 5)
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    for k, name in enumerate(('MASK', 'MIN', 'MAX', 'ABSDIFF', 'BLEND', 'PAIR')):
        assert ("#define VPT_COMBINE_%-7s %d" % (name, k)) in header
    assert "(2^32 - 1) * 65535^2 < 2^64" in header                # the bound of the sums is stated where the entry point is declared


def test_rendering_context_combine_option_is_validated_in_the_constructor():
    spec = vpt_amd.RenderingContext._combine_spec
    reader = object()
    assert spec(None) is None
    assert spec({'reader': reader, 'op': 'min'}) == {'reader': reader, 'volume': None, 'op': 'min', 'channel': 0, 'params': {}, 'resample': None}
    filled = spec({'reader': reader, 'op': 'mask', 'lo': 1, 'hi': 300, 'fill': 9, 'channel': 1, 'resample': 'nearest'})
    assert filled['params'] == {'lo': 1, 'hi': 300, 'fill': 9} and filled['channel'] == 1 and filled['resample'] == 'nearest'
    assert spec({'reader': reader, 'op': 'mask'})['params'] == {'lo': 0, 'hi': None, 'fill': 0}
    assert spec({'reader': reader, 'op': 'blend', 'wa': 512, 'wb': -256})['params'] == {'wa': 512, 'wb': -256, 'offset': 0}
    bad = ['mask', {}, {'op': 'min'}, {'reader': reader}, {'reader': reader, 'volume': reader, 'op': 'min'}, {'volume': reader, 'op': 'min'},
           {'reader': reader, 'op': 'mean'}, {'reader': reader, 'op': 'min', 'lo': 1}, {'reader': reader, 'op': 'mask', 'wa': 1},
           {'reader': reader, 'op': 'mask', 'lo': 5, 'hi': 4}, {'reader': reader, 'op': 'mask', 'hi': 65536}, {'reader': reader, 'op': 'mask', 'fill': -1},
           {'reader': reader, 'op': 'blend'}, {'reader': reader, 'op': 'blend', 'wa': 4097, 'wb': 0}, {'reader': reader, 'op': 'blend', 'wa': 1, 'wb': 1, 'offset': 70000},
           {'reader': reader, 'op': 'min', 'channel': 2}, {'reader': reader, 'op': 'min', 'resample': 'cubic'}, {'reader': reader, 'op': 'min', 'scale': 2}]
    for options in bad:
        with pytest.raises(ValueError):
            spec(options)
    # 'pair' writes the second channel, as gradient, components mode 'label' and distance mode 'channel' do: refused before a device is opened
    pair = {'reader': reader, 'op': 'pair'}
    for other in ({'gradient': 'sobel'}, {'components': {'lo': 1, 'hi': 2, 'mode': 'label'}}, {'distance': {'lo': 1, 'hi': 2, 'mode': 'channel'}}):
        with pytest.raises(ValueError, match="second channel"):
            vpt_amd.RenderingContext(dict(other, combine=pair))


# ---- the JS twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", DTYPES)
def test_node_checks_and_twin_equal_the_numpy_statement(tmp_path, dtype):
    nx, ny, nz = 13, 9, 11
    M = int(np.iinfo(dtype).max)
    _, a, b = value_sets(dtype, (nx, ny, nz), seed=23)[0]
    two = np.stack([b, a], axis=-1)                               # channel 1 of the second volume is a
    little = lambda v: v.astype(v.dtype.newbyteorder('<')).tobytes()
    (tmp_path / "a.raw").write_bytes(little(a)); (tmp_path / "b.raw").write_bytes(little(two))
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_combine_host.js"), str(tmp_path / "a.raw"), str(tmp_path / "b.raw"),
                          str(nx), str(ny), str(nz), str(a.dtype.itemsize * 8)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js combine host ok'
    got = json.loads(lines[-2])
    lo, hi = mask_range(dtype)
    assert got['mask'] == combine_texels(a, two, 'mask', channel=0, lo=lo, hi=hi, fill=M - 1).reshape(-1).tolist()
    for op in ONE_WIDTH_OPS:
        assert got[op] == combine_texels(a, two, op, channel=0).reshape(-1).tolist(), op
    assert got['absdiff1'] == [0] * a.size                        # against channel 1, which is a itself
    for k, (wa, wb, offset) in enumerate(blends(M)):
        assert got['blend'][k] == combine_texels(a, two, 'blend', wa=wa, wb=wb, offset=offset).reshape(-1).tolist(), (wa, wb, offset)
    want = compare_stats(a, two, (lo, hi), (lo, hi))
    assert {k: int(got['compare'][k]) for k in STATS} == {k: want[k] for k in STATS}
    for k in ('dice', 'jaccard', 'mse'):                          # IEEE double, the same operations in the same order
        assert got['compare'][k] == want[k], k
    assert math.isclose(got['compare']['psnr'], want['psnr'], rel_tol=1e-14)      # log10 is not correctly rounded in either library
    same = got['compare_same']
    assert same['psnr'] is None and same['mse'] == 0 and int(same['differing']) == 0
