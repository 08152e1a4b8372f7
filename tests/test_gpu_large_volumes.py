"""GPU: the volume operations in front of the renderers on volumes of more than 2^31 (tier A) and more than 2^32 (tier B) voxels, where a
linear index, a byte offset or a counter kept in 32 bits goes wrong.

The volumes are sparse (tests/large_volumes.py): noise in a slab at z = 0, in one straddling the plane of linear voxel index 2^31 (and of
2^30 where four-byte values pass byte offset 2^32), and in one ending at z = nz - 1; background 0 elsewhere.  Every operation is held,
byte for byte, to its numpy statement applied to the small twin of the slabs (tests/test_large_volumes_host.py shows, on small shapes, that
the statement on the twin is the statement on the whole volume there).  Whole planes come back through the contiguous copy, a box with
x0, y0 > 0 at the far slab through k_read_block / k_read_field; background planes between the slabs are read too.

Each test states its peak device memory as the sum of what it allocates (GiB; a volume = linear storage + bricks + boundary atlas:
large_volumes.volume_bytes) and skips, with both figures, when less is free.  Nothing else may skip."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.distance import NONE
from vpt_amd.resample import nearest_index

from large_volumes import (TIER_A, TIER_B, GIB, REACH, Layout, voxels, volume_bytes, field_bytes, sparse_volume, planes, differences,
                           distance_squared_within, slab_distances, counts)

pytestmark = pytest.mark.gpu

KINDS = ('aligned', 'odd')
DTYPE = {8: np.uint8, 16: np.uint16}


def require(need):
    """skips when fewer than `need` bytes of device memory are free"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("the test allocates %.1f GiB of device memory at its peak, %.1f GiB are free" % (need / GIB, free / GIB))


def tier(shape, above, below=None):
    """the product of the shape, checked on the CPU"""
    n = voxels(shape)
    assert n > above and (below is None or n < below), "%r has %d voxels" % (shape, n)
    assert max(shape) <= 4096
    return n


def hold(out, want, windows, what):
    """the planes of every window of the volume `out` equal the twin's; at the far slab also a box that is not whole planes"""
    d = out.modality['dimensions']
    assert (d['width'], d['height']) == want.shape[1:3][::-1], what
    for z_lo, z_hi, t_lo in windows:
        expected = want[t_lo:t_lo + (z_hi - z_lo)]
        assert len(np.unique(expected)) >= 8, "degenerate input: %d distinct values expected in planes %d .. %d" % (len(np.unique(expected)), z_lo, z_hi - 1)
        differences(planes(out, z_lo, z_hi), expected, "%s, planes %d .. %d" % (what, z_lo, z_hi - 1))
    z_lo, z_hi, t_lo = windows[-1]
    x0, y0, w, h = 5, 3, d['width'] - 9, 7
    box = out.read_block(x0, y0, z_lo, w, h, z_hi - z_lo)
    differences(box, np.ascontiguousarray(want[t_lo:t_lo + (z_hi - z_lo), y0:y0 + h, x0:x0 + w]), "%s, a box of the far slab" % what)


def background(out, zs, value, what):
    for z in zs:
        plane = planes(out, z, z + 1)
        assert (plane == value).all(), "%s: plane %d between the slabs is not %r everywhere" % (what, z, value)


def refused(call, *needles):
    with pytest.raises(vpt_amd.VptError) as e:
        call()
    assert e.value.code == N.ERR_UNSUPPORTED, str(e.value)
    for needle in needles:
        assert needle in str(e.value), str(e.value)


# ---- window and range ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_window_of_more_than_2_32_voxels(gpu_ctx, kind, bits):
    """R8 -> R8 / R16 at tier B.  Peak: source 19.9 + result 19.9 (R8) or 40.2 (R16) = 39.8 / 60.1 GiB.  The window begins below 0, so
    the background is not 0 in the result; the result's range() sees it."""
    shape = TIER_B[kind]
    tier(shape, 1 << 32)
    require(volume_bytes(shape, 1) + volume_bytes(shape, bits // 8))
    lay = Layout(shape, 2, 1)
    blocks = lay.noise(np.uint8, 11)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.window(-16, 200, 'r%d' % bits)
    finally:
        src.destroy()
    try:
        want = vpt_amd.window_texels(lay.twin(blocks), -16, 200, bits)
        floor = int(vpt_amd.window_texels(np.zeros((1, 1, 1), np.uint8), -16, 200, bits)[0, 0, 0])
        assert floor > 0
        hold(out, want, lay.windows(), "window R8 -> R%d %s" % (bits, kind))
        background(out, lay.between(), floor, "window")
        assert out.range() == (floor, (1 << bits) - 1)
    finally:
        out.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_window_r16_to_r8_past_byte_2_32(gpu_ctx, kind):
    """R16 -> R8 at tier A: the source's byte offsets pass 2^32 at voxel 2^31.  Peak: source 21.4 + result 10.6 = 32.0 GiB."""
    shape = TIER_A[kind]
    tier(shape, 1 << 31, 1 << 32)
    require(volume_bytes(shape, 2) + volume_bytes(shape, 1))
    lay = Layout(shape, 2, 1, marks=(1 << 30, 1 << 31))
    blocks = lay.noise(np.uint16, 21)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.window(1000, 60000, 'r8')
    finally:
        src.destroy()
    try:
        hold(out, vpt_amd.window_texels(lay.twin(blocks), 1000, 60000, 8), lay.windows(), "window R16 -> R8 %s" % kind)
        background(out, lay.between(), 0, "window")
    finally:
        out.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("bits,kind", [(8, 'odd'), (16, 'aligned')])
def test_range_with_the_extremes_in_the_far_slab_only(gpu_ctx, bits, kind):
    """range() of an R8 volume at tier B and an R16 volume at tier A whose background is the image of code 0 under a window that begins
    below 0 (7 in R8, 1751 in R16) and whose only 0 and only largest code lie in the far slab.  Peak: two R8 volumes at tier B, 39.8 GiB;
    at tier A R8 10.6 + R16 21.4 = 32.0 GiB."""
    shape = (TIER_B if bits == 8 else TIER_A)[kind]
    n = tier(shape, 1 << 32) if bits == 8 else tier(shape, 1 << 31, 1 << 32)
    require(volume_bytes(shape, 1) + volume_bytes(shape, bits // 8))
    nx, ny, nz = shape
    M = (1 << bits) - 1
    lay = Layout(shape, 2, 1)
    blocks = [np.minimum(b, 254) for b in lay.noise(np.uint8, 31)]
    blocks[-1][1, ny - 2, nx - 3] = 255                              # the only code that the window takes to M
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.window(-7, 255, 'r%d' % bits)
    finally:
        src.destroy()
    try:
        floor = int(vpt_amd.window_texels(np.zeros((1, 1, 1), np.uint8), -7, 255, bits)[0, 0, 0])
        want = vpt_amd.window_texels(lay.twin(blocks), -7, 255, bits)
        assert floor > 0 and int(want.min()) == floor and (want == M).sum() == 1
        assert ((nz - 1) * ny + ny - 2) * nx + nx - 3 > n - nx * ny > (1 << 31)
        assert out.range() == (floor, M)
        out.upload_block(nx - 5, ny - 4, nz - 2, np.zeros((1, 1, 1), DTYPE[bits]))      # the only 0, in the far slab too
        assert out.range() == (0, M)
        out.upload_block(nx - 3, ny - 2, nz - 1, np.full((1, 1, 1), floor, DTYPE[bits]))
        assert out.range() == (0, int(want[want < M].max()))
    finally:
        out.destroy()


# ---- smoothing, rank filters, the gradient ---------------------------------------------------------------------------------------
def local(ctx, kind, thick, halo, derive, statement, what, seed):
    shape = TIER_B[kind]
    tier(shape, 1 << 32)
    lay = Layout(shape, thick, 2 * halo)
    blocks = lay.noise(np.uint8, seed)
    src = sparse_volume(ctx, lay, blocks)
    try:
        out = derive(src)
    finally:
        src.destroy()
    try:
        hold(out, statement(lay.twin(blocks)), lay.windows(halo), "%s %s" % (what, kind))
        background(out, lay.between(halo), 0, what)
    finally:
        out.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_smooth_of_more_than_2_32_voxels(gpu_ctx, kind, passes):
    """Peak: source 19.9 + result 19.9 (+ the scratch of two passes, 4.0) = 39.8 / 43.8 GiB."""
    shape = TIER_B[kind]
    require(2 * volume_bytes(shape, 1) + (voxels(shape) if passes > 1 else 0))
    local(gpu_ctx, kind, 3, passes, lambda v: v.smooth(passes), lambda a: vpt_amd.smooth_texels(a, passes), "smooth(%d)" % passes, 41)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("op", ['median', 'erode'])
@pytest.mark.parametrize("kind", KINDS)
def test_rank_filters_of_more_than_2_32_voxels(gpu_ctx, kind, op):
    """Peak: source 19.9 + result 19.9 = 39.8 GiB.  (The median's numpy statement takes seconds on the twin's 13 planes of 2^20 voxels.)"""
    require(2 * volume_bytes(TIER_B[kind], 1))
    local(gpu_ctx, kind, 3, 1, lambda v: v.rank(op), lambda a: vpt_amd.rank_texels(a, op), op, 51)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("operator", ['central', 'sobel'])
@pytest.mark.parametrize("kind", KINDS)
def test_gradient_of_more_than_2_32_voxels(gpu_ctx, kind, operator):
    """The RG8 result's byte offsets pass 2^32 at voxel 2^31 and 2^33 at voxel 2^32.  Peak: source 19.9 + result 39.8 = 59.7 GiB."""
    shape = TIER_B[kind]
    require(volume_bytes(shape, 1) + volume_bytes(shape, 1, 2))

    def statement(a):
        return np.ascontiguousarray(np.stack([a, vpt_amd.gradient_magnitude(a, operator, 1.0)], axis=-1))
    local(gpu_ctx, kind, 3, 1, lambda v: v.derive_gradient(operator, 1.0), statement, "gradient %s" % operator, 61)


# ---- the 2x reduction ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_reduce_of_more_than_2_32_voxels(gpu_ctx, kind):
    """Both forms run: the 16-byte chunks of the aligned shape (33 x 498 x 2048 of them, below the 2^32 that launch_reduce refuses) and the
    texel-by-texel form of the odd one (538 M result texels, 2.1 M workgroups, below the 2^31 it refuses).  Peak: source 19.9 + result 2.6 =
    22.5 GiB."""
    shape = TIER_B[kind]
    tier(shape, 1 << 32)
    nx, ny, nz = shape
    half = ((nx + 1) // 2, (ny + 1) // 2, nz // 2)
    assert (nx % 32 == 0) == (kind == 'aligned') and (voxels(half) + 255) // 256 <= 0x7fffffff
    require(volume_bytes(shape, 1) + volume_bytes(half, 1))
    lay = Layout(shape, 4, 2, even=True)
    blocks = lay.noise(np.uint8, 71)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.reduce()
    finally:
        src.destroy()
    try:
        assert out.modality['dimensions'] == {'width': half[0], 'height': half[1], 'depth': half[2]}
        hold(out, vpt_amd.reduce_texels(lay.twin(blocks)), lay.halved(), "reduce %s" % kind)
        background(out, [z // 2 for z in lay.between(2)], 0, "reduce")
    finally:
        out.destroy()


# ---- histograms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("bits,kind", [(8, 'aligned'), (8, 'odd'), (16, 'aligned'), (16, 'odd')])
def test_histograms_with_a_bin_above_2_31(gpu_ctx, bits, kind):
    """Tier A: the background bin holds more than 2^31 voxels and every bin is exact.  Peak: one R8 / R16 volume, 10.6 / 21.4 GiB."""
    shape = TIER_A[kind]
    n = tier(shape, 1 << 31, 1 << 32)
    require(volume_bytes(shape, bits // 8))
    lay = Layout(shape, 2, 1, marks=(1 << 30, 1 << 31))
    blocks = lay.noise(DTYPE[bits], 81)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        coarse, fine = src.histogram(), src.code_histogram()
    finally:
        src.destroy()
    want = counts(blocks, 256, bits - 8, n)
    assert want[0] > (1 << 31) and want.sum() == n
    differences(coarse.astype(np.int64), want, "histogram R%d %s" % (bits, kind))
    differences(fine.astype(np.int64), counts(blocks, 1 << bits, 0, n), "code histogram R%d %s" % (bits, kind))


@pytest.mark.timeout(120)
def test_histogram_of_a_gradient_volume_with_a_bin_above_2_31(gpu_ctx):
    """Tier A, RG8 (k_histogram_rg): bin [0][0] holds the background.  Peak: source 10.6 + result 21.2 = 31.8 GiB."""
    shape = TIER_A['odd']
    n = tier(shape, 1 << 31, 1 << 32)
    require(volume_bytes(shape, 1) + volume_bytes(shape, 1, 2))
    lay = Layout(shape, 2, 2)
    blocks = lay.noise(np.uint8, 91)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.derive_gradient('central', 1.0)
    finally:
        src.destroy()
    try:
        got = out.histogram()
    finally:
        out.destroy()
    twin = lay.twin(blocks)
    g = vpt_amd.gradient_magnitude(twin, 'central', 1.0)
    want = np.zeros((256, 256), np.int64)
    inside = 0
    for z_lo, z_hi, t_lo in lay.windows(1):
        sl = slice(t_lo, t_lo + z_hi - z_lo)
        want += np.bincount(g[sl].reshape(-1).astype(np.int64) * 256 + twin[sl].reshape(-1), minlength=65536).reshape(256, 256)
        inside += g[sl].size
    want[0, 0] += n - inside
    assert want[0, 0] > (1 << 31)
    differences(got.astype(np.int64), want, "histogram RG8")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_histograms_refuse_more_than_2_32_voxels(gpu_ctx, kind):
    """Tier B: the 32-bit background bin of such a volume would wrap (it came back modulo 2^32 with VPT_OK before the guard); both
    histograms refuse, as components does.  Peak: one R8 volume, 19.9 GiB."""
    shape = TIER_B[kind]
    n = tier(shape, 1 << 32)
    require(volume_bytes(shape, 1))
    lay = Layout(shape, 2, 1)
    blocks = lay.noise(np.uint8, 101)
    assert n - sum(b.size for b in blocks) > 0xFFFFFFFF              # what the background bin would have to hold
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        refused(src.histogram, str(n), "32-bit")
        refused(src.code_histogram, str(n), "32-bit")
        refused(src.percentile_window, str(n), "32-bit")              # what a rendering context with a window in percentiles calls
        refused(lambda: src.components(250, 255), str(n), "32-bit")
    finally:
        src.destroy()


# ---- upload into and read-back from an existing large volume ---------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("bits,kind", [(8, 'odd'), (16, 'aligned')])
def test_upload_block_into_the_far_end(gpu_ctx, bits, kind):
    """A box with x0, y0 > 0 behind voxel 2^32 (R8, tier B) / behind byte 2^32 (R16, tier A) goes in through k_blit_block and comes back
    through k_read_block; the slab in front of it is unchanged; a window derived afterwards sees it.  Peak: source 19.9 + window 19.9 =
    39.8 GiB (R8); 21.4 + 10.6 = 32.0 GiB (R16)."""
    shape = (TIER_B if bits == 8 else TIER_A)[kind]
    tier(shape, 1 << 32) if bits == 8 else tier(shape, 1 << 31, 1 << 32)
    require(volume_bytes(shape, bits // 8) + volume_bytes(shape, 1))
    nx, ny, nz = shape
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = Layout(shape, 2, 1)
    blocks = lay.noise(dtype, 111)
    box = np.random.default_rng(112).integers(0, M + 1, size=(2, 9, nx - 11)).astype(dtype)
    x0, y0, z0 = 6, ny - 13, nz - 4                                   # the two planes in front of the far slab, which is planes nz - 2, nz - 1
    assert ((z0 * ny + y0) * nx + x0) * (bits // 8) > (1 << 32)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        src.upload_block(x0, y0, z0, box)
        differences(src.read_block(x0, y0, z0, box.shape[2], box.shape[1], box.shape[0]), box, "the uploaded box")
        want = np.zeros((2, ny, nx), dtype)
        want[:, y0:y0 + 9, x0:x0 + box.shape[2]] = box
        differences(planes(src, z0, z0 + 2), want, "the planes of the box")
        assert not planes(src, z0 - 1, z0).any()
        for (z_lo, z_hi, _), block in zip(lay.windows(), blocks):
            differences(planes(src, z_lo, z_hi), block, "a slab after the upload")
        out = src.window(0, M, 'r8')
    finally:
        src.destroy()
    try:
        differences(planes(out, z0, z0 + 2), vpt_amd.window_texels(want, 0, M, 8), "the window of the uploaded box")
    finally:
        out.destroy()


# ---- connected components --------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(180)
@pytest.mark.parametrize("bits,kind,connectivity", [(16, 'aligned', 6), (8, 'odd', 26)])
def test_components_of_more_than_2_31_voxels(gpu_ctx, bits, kind, connectivity):
    """Tier A, the largest that 32-bit labels admit.  A background plane parts the twin's slabs as thousands part the volume's, so the
    components, their voxel counts and their order (by count, then by first voxel, which is monotone in z) are the same; the first voxels
    are the volume's own.  Peak, R16: source 21.4 + handle 15.0 + the count array 10.0 = 46.4 GiB while labelling, then handle 15.0 +
    label volume (RG16) 42.7 = 57.7 GiB.  R8: 10.6 + 12.5 + 10.0 = 33.1, then 12.5 + 21.2 = 33.7 GiB."""
    shape = TIER_A[kind]
    n = tier(shape, 1 << 31, 0xFFFFFFFE)
    nx, ny, nz = shape
    item = bits // 8
    require(max(volume_bytes(shape, item) + field_bytes(shape, item) + 4 * n, field_bytes(shape, item) + volume_bytes(shape, item, 2)))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lo = M - (M + 1) // 16 + 1                                        # the top sixteenth of the codes: small components, thousands of them
    lay = Layout(shape, 2, 1, marks=(1 << 30, 1 << 31))
    blocks = lay.noise(dtype, 121)
    twin = lay.twin(blocks)
    ranks, listed = vpt_amd.components_texels(twin, lo, M, connectivity)
    listed = [(x, y, lay.to_volume(z), v) for x, y, z, v in listed]
    far = [c for c in listed if (c[2] * ny + c[1]) * nx + c[0] > (1 << 31)]
    assert len(listed) >= 4 and len({c[2] for c in listed}) >= 2 and len(far) >= 1 and len({c[3] for c in listed}) >= 4
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.components(lo, M, connectivity)
    finally:
        src.destroy()
    try:
        foreground = int(sum(((b >= lo).sum() for b in blocks)))
        assert found.info == {'listed': len(listed), 'dropped': 0, 'foreground_voxels': foreground, 'listed_voxels': foreground}
        assert found.list() == listed
        x0, y0, w, h = 5, 3, nx - 9, 7
        for z_lo, z_hi, t_lo in lay.windows():
            differences(found.ranks(0, 0, z_lo, nx, ny, z_hi - z_lo), ranks[t_lo:t_lo + z_hi - z_lo], "ranks, planes %d .. %d" % (z_lo, z_hi - 1))
            differences(found.ranks(x0, y0, z_lo, w, h, z_hi - z_lo), np.ascontiguousarray(ranks[t_lo:t_lo + z_hi - z_lo, y0:y0 + h, x0:x0 + w]),
                        "a box of ranks, planes %d .. %d" % (z_lo, z_hi - 1))
        for z in lay.between():
            assert not found.ranks(0, 0, z, nx, ny, 1).any() and not found.ranks(x0, y0, z, w, h, 1).any()
        k = len(listed) // 2
        kept = found.keep(1, k)
        try:
            hold(kept, vpt_amd.keep_texels(twin, ranks, 1, k), lay.windows(), "keep(1, %d)" % k)
            background(kept, lay.between(), 0, "keep")
        finally:
            kept.destroy()
        pair = found.label()
        try:
            hold(pair, vpt_amd.label_texels(twin, ranks), lay.windows(), "label")
            background(pair, lay.between(), 0, "label")
        finally:
            pair.destroy()
    finally:
        found.destroy()


# ---- the distance transform ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(180)
@pytest.mark.parametrize("bits,kind", [(8, 'aligned'), (8, 'odd'), (16, 'odd')])
def test_distance_to_a_range_in_large_volumes(gpu_ctx, bits, kind):
    """seeds 'range': R8 at tier B, R16 at tier A; the seeds are the top codes, 3 % of a slab's voxels.  Peak, tier B: source 19.9 + handle
    20.0 + the `other` and `stack` buffers 2 x 16.0 = 71.9 GiB while transforming, then handle 20.0 + channel volume (RG8) 39.8 = 59.8 GiB.
    Tier A R16: 21.4 + 15.0 + 2 x 10.0 = 56.4, then 15.0 + 42.7 = 57.7 GiB."""
    shape = (TIER_B if bits == 8 else TIER_A)[kind]
    n = tier(shape, 1 << 32) if bits == 8 else tier(shape, 1 << 31, 1 << 32)
    nx, ny, nz = shape
    item = bits // 8
    require(max(volume_bytes(shape, item) + field_bytes(shape, item) + 8 * n, field_bytes(shape, item) + volume_bytes(shape, item, 2)))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lo = M - (M + 1) // 32 + 1                                        # 1 / 32 of the codes
    lay = Layout(shape, 3, REACH + 1, marks=(1 << 31,) if bits == 8 else (1 << 30, 1 << 31))      # four-byte values pass byte 2^32 at voxel 2^30
    blocks = lay.noise(dtype, 131)
    d2, largest = slab_distances(lay, blocks, lo, M)
    seeds = int(sum((b >= lo).sum() for b in blocks))
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.distance(lo, M, 'range')
    finally:
        src.destroy()
    try:
        assert found.info['seeds'] == seeds
        x0, y0, w, h = 5, 3, nx - 9, 7
        for (z_lo, z_hi, _), want in zip(lay.windows(), d2):
            assert len(np.unique(want)) >= 8
            differences(found.squared(0, 0, z_lo, nx, ny, z_hi - z_lo), want, "squared, planes %d .. %d" % (z_lo, z_hi - 1))
            differences(found.squared(x0, y0, z_lo, w, h, z_hi - z_lo), np.ascontiguousarray(want[:, y0:y0 + h, x0:x0 + w]),
                        "a box of squared distances, planes %d .. %d" % (z_lo, z_hi - 1))
        # midway between the last two slabs: at least the squared distance to the nearer slab's nearest plane, and in a box the minimum
        # over the seeds of both
        a, b = lay.starts[-2] + lay.thick - 1, lay.starts[-1]
        z = (a + b) // 2
        plane = found.squared(0, 0, z, nx, ny, 1)
        assert int(plane.min()) >= min(z - a, b - z) ** 2 and int(plane.max()) < NONE
        bx, by = nx - 12, ny - 10
        got = found.squared(bx, by, z, 6, 4, 1)
        at = [np.nonzero(blk >= lo) for blk in blocks[-2:]]
        sz = np.concatenate([c[0] + z0 for c, z0 in zip(at, lay.starts[-2:])]).astype(np.int64)
        sy, sx = (np.concatenate([c[k] for c in at]).astype(np.int64) for k in (1, 2))
        want = np.empty((1, 4, 6), np.uint32)
        for j in range(4):
            for i in range(6):
                want[0, j, i] = ((sx - (bx + i)) ** 2 + (sy - (by + j)) ** 2 + (sz - z) ** 2).min()
        differences(got, want, "a box of the plane midway between the last two slabs")
        assert found.info['largest'] >= int(plane.max())
        near = found.within(1, largest // 2, 3)
        try:
            for (z_lo, z_hi, _), block, want in zip(lay.windows(), blocks, d2):
                differences(planes(near, z_lo, z_hi), vpt_amd.within_texels(block, want, 1, largest // 2, 3), "within, planes %d .. %d" % (z_lo, z_hi - 1))
            differences(near.read_block(x0, y0, lay.starts[-1], w, h, lay.thick),
                        np.ascontiguousarray(vpt_amd.within_texels(blocks[-1], d2[-1], 1, largest // 2, 3)[:, y0:y0 + h, x0:x0 + w]), "a box of within")
            background(near, [z], 3, "within")
        finally:
            near.destroy()
        pair = found.channel(16)
        try:
            for (z_lo, z_hi, _), block, want in zip(lay.windows(), blocks, d2):
                differences(planes(pair, z_lo, z_hi), vpt_amd.channel_texels(block, want, 16), "channel, planes %d .. %d" % (z_lo, z_hi - 1))
            differences(pair.read_block(x0, y0, lay.starts[-1], w, h, lay.thick),
                        np.ascontiguousarray(vpt_amd.channel_texels(blocks[-1], d2[-1], 16)[:, y0:y0 + h, x0:x0 + w]), "a box of channel")
        finally:
            pair.destroy()
    finally:
        found.destroy()


@pytest.mark.timeout(180)
def test_distance_to_the_rest_counts_more_than_2_32_seeds(gpu_ctx):
    """seeds 'rest' at tier B: every voxel but the slabs' top codes is a seed, more than 2^32 of them; the count arrives intact.  Peak:
    source 19.9 + handle 20.0 + 2 x 16.0 = 71.9 GiB."""
    shape = TIER_B['odd']
    n = tier(shape, 1 << 32)
    nx, ny, nz = shape
    require(volume_bytes(shape, 1) + field_bytes(shape, 1) + 8 * n)
    lay = Layout(shape, 3, 4)
    blocks = lay.noise(np.uint8, 141)
    lo = 48                                                           # 13 / 16 of a slab's voxels are no seeds: depths of up to three voxels
    seeds = n - int(sum((b >= lo).sum() for b in blocks))
    assert seeds > (1 << 32)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.distance(lo, 255, 'rest')
    finally:
        src.destroy()
    try:
        assert found.info['seeds'] == seeds
        # the far slab with the background plane in front of it (all seeds): nothing lies behind it
        padded = np.concatenate([np.zeros((1, ny, nx), np.uint8), blocks[-1]])
        want = distance_squared_within(padded < lo, 4)[1:]
        assert int(want.max()) <= 4 * 4 + 2 * 4 and len(np.unique(want)) >= 8
        z0 = lay.starts[-1]
        differences(found.squared(0, 0, z0, nx, ny, lay.thick), want, "squared, the far slab")
        differences(found.squared(5, 3, z0, nx - 9, 7, lay.thick), np.ascontiguousarray(want[:, 3:10, 5:nx - 4]), "a box of squared distances, the far slab")
        assert not found.squared(0, 0, lay.between()[-1], nx, ny, 1).any()
    finally:
        found.destroy()


# ---- resampling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", KINDS)
def test_resample_nearest_to_more_than_2_32_voxels_and_down(gpu_ctx, kind):
    """'nearest' from tier B to a result that has more than 2^32 voxels itself (other x and y sizes, nz kept: plane Z copies plane Z), and
    down to a third of x and y and half of z, whose last plane comes from the far slab.  Peak: source 19.9 + result 20.1 = 40.0 GiB."""
    shape = TIER_B[kind]
    tier(shape, 1 << 32)
    nx, ny, nz = shape
    big = (1060, 993, nz) if kind == 'aligned' else (1027, 1025, nz)      # a row of whole dwords (four texels a lane) / texel by texel
    tier(big, 1 << 32)
    require(volume_bytes(shape, 1) + volume_bytes(big, 1))
    lay = Layout(shape, 2, 1)
    blocks = lay.noise(np.uint8, 151)
    twin = lay.twin(blocks)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.resample(*big, mode='nearest')
        try:
            want = vpt_amd.resample_texels(twin, (twin.shape[0], big[1], big[0]), 'nearest')      # z: the identity
            hold(out, want, lay.windows(), "nearest, %s to %r" % (kind, big))
            background(out, lay.between(), 0, "nearest")
        finally:
            out.destroy()
        small = (nx // 3, ny // 3, 2048)                              # plane Z copies plane 2 Z + 1: the odd planes of every slab, 4095 the last
        out = src.resample(*small, mode='nearest')
        try:
            jx = nearest_index(nx, small[0])
            jy = nearest_index(ny, small[1])
            for z0, block in zip(lay.starts, blocks):
                for z in range(z0, z0 + lay.thick):
                    if z % 2 == 1:
                        want = np.ascontiguousarray(block[z - z0][jy][:, jx]).reshape(1, small[1], small[0])
                        assert len(np.unique(want)) >= 8
                        differences(planes(out, z // 2, z // 2 + 1), want, "nearest down, plane %d from plane %d" % (z // 2, z))
            differences(out.read_block(5, 3, 2047, small[0] - 9, 7, 1), np.ascontiguousarray(block[-1][jy][:, jx][3:10, 5:small[0] - 4]).reshape(1, 7, small[0] - 9),
                        "a box of the last plane")
        finally:
            out.destroy()
    finally:
        src.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind,width,height,slabs", [('aligned', 96, 1030, 3), ('odd', 96, 1030, 3), ('odd', 1060, 300, 2)])
def test_resample_filtered_in_the_plane_of_more_than_2_32_voxels(gpu_ctx, kind, width, height, slabs):
    """'filtered' from tier B with nz kept and x and y changed: every plane is a 2-D resample of its own, so the twin (single planes) is
    exact.  96 x 1030: x shrinks, y grows.  1060 x 300: x grows, so the workspace of the row pass has more than 2^32 entries itself; its
    numpy statement takes seconds a plane, so only the planes at voxel 2^31 and at the far end are held.  The workspace is 4 bytes x result
    width x source ny x nz x channels: 1.5 GiB at 96, 16.6 GiB at 1060.  Peak: source 19.9 + workspace 16.6 + result (1060 x 300 x 4096:
    6.1) = 42.6 GiB; at 96: 19.9 + 1.5 + 2.0 = 23.4 GiB."""
    shape = TIER_B[kind]
    tier(shape, 1 << 32)
    nx, ny, nz = shape
    assert (4 * width * ny * nz > (1 << 34)) == (width > nx)          # more than 2^32 dwords of workspace
    require(volume_bytes(shape, 1) + 4 * width * ny * nz + volume_bytes((width, height, nz), 1))
    lay = Layout(shape, 1, 0)                                         # single planes; the twin is the three of them
    blocks = lay.noise(np.uint8, 161)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.resample(width, height, nz, mode='filtered')
    finally:
        src.destroy()
    try:
        twin = lay.twin(blocks)[-slabs:]
        windows = [(z_lo, z_hi, t_lo - (3 - slabs)) for z_lo, z_hi, t_lo in lay.windows()[-slabs:]]
        hold(out, vpt_amd.resample_texels(twin, (slabs, height, width), 'filtered'), windows, "filtered, %s to %d x %d" % (kind, width, height))
        background(out, lay.between() + [1], 0, "filtered")
    finally:
        out.destroy()


@pytest.mark.timeout(120)
def test_resample_filtered_along_z_of_more_than_2_31_voxels(gpu_ctx):
    """'filtered' from an R16 volume at tier A (source bytes past 2^32) to 96 x 80 x 1024: a result plane averages 4 source planes.  The
    slabs are 4 planes thick and begin on multiples of 4, so result plane Z is resample_texels of exactly the planes 4 Z .. 4 Z + 3.
    Workspace: 4 x 96 x 809 x 4096 = 1.2 GiB.  Peak: source 21.4 + workspace 1.2 + result 0.1 = 22.7 GiB."""
    shape = TIER_A['odd']
    tier(shape, 1 << 31, 1 << 32)
    nx, ny, nz = shape
    require(volume_bytes(shape, 2) + 4 * 96 * ny * nz + volume_bytes((96, 80, 1024), 2))
    lay = Layout(shape, 4, 4, even=True)
    p = (1 << 31) // (nx * ny)
    lay.starts = [0, p - p % 4, nz - 4]                               # whole cells of four planes
    assert lay.starts[1] * nx * ny <= (1 << 31) < (lay.starts[1] + 4) * nx * ny
    blocks = lay.noise(np.uint16, 171)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.resample(96, 80, 1024, mode='filtered')
    finally:
        src.destroy()
    try:
        for z0, block in zip(lay.starts, blocks):
            want = vpt_amd.resample_texels(block, (1, 80, 96), 'filtered')
            assert len(np.unique(want)) >= 8
            differences(planes(out, z0 // 4, z0 // 4 + 1), want, "filtered along z, plane %d" % (z0 // 4))
            if z0 == nz - 4:
                differences(out.read_block(5, 3, 1023, 96 - 9, 7, 1), np.ascontiguousarray(want[:, 3:10, 5:96 - 4]), "a box of the last plane")
        background(out, [z0 // 4 + 1 for z0 in lay.starts[:-1]] + [1022], 0, "filtered along z")
    finally:
        out.destroy()
