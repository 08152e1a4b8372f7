"""Grey-level morphological reconstruction of a marker under a mask, and the geodesic operations that are one reconstruction each, on the
host: the numpy statement of the contract the device kernels (vpt_volume_reconstruct, vpt_volume_geodesic; include/vpt.h) are held to, for
callers without a device and as the contract's documentation.

``marker`` and ``mask`` are [depth][height][width] uint8 or uint16 arrays of one type and shape, or [depth][height][width][2] with a channel
argument naming the channel that is read.  All compares are unsigned on whole codes, M = 255 / 65535.  Connectivity c is 6 (voxels that
share a face), 18 (a face or an edge) or 26 (a face, an edge or a corner); a neighbour outside the volume does not exist.

  dilation:  r0 = min(marker, mask);  r_k+1(v) = min(mask(v), max(r_k(v), max over the c-neighbours u of v of r_k(u)));  the result is the
             first r_k with r_k+1 = r_k.  Equivalently R(v) = max over all voxels s and all c-connected paths from s to v of
             min(r0(s), min of the mask along the path), so the result is unique.
  erosion:   R_e(marker, mask) = M - R_d(M - marker, M - mask): r0 = max(marker, mask), min and max exchanged.

  fill_holes    R_e(m, src), m = src on the voxels of the volume's six faces, M elsewhere
  clear_border  src - R_d(m, src), m = src on the six faces, 0 elsewhere
  hmax          R_d(max(src - h, 0), src); h = 0 gives src
  hmin          R_e(min(src + h, M), src)
  dome          src - hmax_h(src)
  maxima        M where src > hmax_1(src), 0 elsewhere: the plateaus without a higher c-neighbour; a voxel of code 0 is never a maximum
  minima        M where src < hmin_1(src), 0 elsewhere; a voxel of code M is never a minimum
The functions iterate the definition to its fixed point: plain, and as slow as the longest path is long."""
import numpy as np

from .components import check_connectivity, neighbour_offsets

RECONSTRUCT_OPS = {'dilation': 0, 'erosion': 1}                                                      # VPT_RECONSTRUCT_*
GEODESIC_OPS = {'fill_holes': 0, 'clear_border': 1, 'hmax': 2, 'hmin': 3, 'dome': 4, 'maxima': 5, 'minima': 6}      # VPT_GEODESIC_*
TAKES_H = ('hmax', 'hmin', 'dome')


def _integer(value):
    return isinstance(value, (int, np.integer)) and not isinstance(value, bool)


def check_reconstruct_op(op):
    """the code of 'dilation' | 'erosion' (VPT_RECONSTRUCT_*); raises ValueError otherwise"""
    if not isinstance(op, str) or op not in RECONSTRUCT_OPS:
        raise ValueError("reconstruct op is 'dilation' or 'erosion', not %r" % (op,))
    return RECONSTRUCT_OPS[op]


def check_geodesic_op(op):
    """the code of 'fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima' (VPT_GEODESIC_*); raises ValueError
    otherwise"""
    if not isinstance(op, str) or op not in GEODESIC_OPS:
        raise ValueError("geodesic op is 'fill_holes', 'clear_border', 'hmax', 'hmin', 'dome', 'maxima' or 'minima', not %r" % (op,))
    return GEODESIC_OPS[op]


def check_h(op, h, largest):
    """``h`` of the geodesic operation ``op`` as an int: 0 .. ``largest`` for 'hmax', 'hmin' and 'dome', 0 for the others; raises
    ValueError otherwise"""
    check_geodesic_op(op)
    if not _integer(h) or not 0 <= h <= largest:
        raise ValueError('geodesic h is an integer in 0 .. %d, not %r' % (largest, h))
    if op not in TAKES_H and h != 0:
        raise ValueError("geodesic op %r takes no h (0), not %r" % (op, h))
    return int(h)


def check_source_channel(channel, channels):
    """``channel`` of a source of ``channels`` channels as an int: 0, or 1 of a two-channel source; raises ValueError otherwise"""
    if not _integer(channel) or channel not in (0, 1):
        raise ValueError('channel is 0 or 1, not %r' % (channel,))
    if channel == 1 and channels != 2:
        raise ValueError('channel 1 needs a two-channel volume')
    return int(channel)


def _channel(array, channel, what):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim not in (3, 4) or (array.ndim == 4 and array.shape[3] != 2):
        raise ValueError('%s is a [depth][height][width] or [depth][height][width][2] uint8 or uint16 array' % what)
    channel = check_source_channel(channel, 2 if array.ndim == 4 else 1)
    return array[..., channel] if array.ndim == 4 else array


def _dilate_under(r, mask, offsets):
    """the fixed point of r <- min(mask, max of r and its neighbours) from r <= mask; int64 arrays"""
    d, h, w = r.shape
    while True:
        p = np.zeros((d + 2, h + 2, w + 2), dtype=r.dtype)         # a neighbour outside the volume reads as 0, which max ignores
        p[1:-1, 1:-1, 1:-1] = r
        grown = r
        for dz, dy, dx in offsets:
            grown = np.maximum(grown, p[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w])
        grown = np.minimum(grown, mask)
        if np.array_equal(grown, r):
            return r
        r = grown


def _reconstruct(marker, mask, erosion, connectivity):
    """marker and mask: arrays of one unsigned type and shape"""
    largest = int(np.iinfo(mask.dtype).max)
    a, b = marker.astype(np.int64), mask.astype(np.int64)
    if erosion:
        a, b = largest - a, largest - b
    r = _dilate_under(np.minimum(a, b), b, neighbour_offsets(connectivity))
    return (largest - r if erosion else r).astype(mask.dtype)


def reconstruct_texels(marker, mask, op='dilation', connectivity=6, channel=0, mask_channel=0):
    """the texels vpt_volume_reconstruct gives for the arrays ``marker`` and ``mask`` (module docstring): a [depth][height][width] array of
    their type"""
    code = check_reconstruct_op(op)
    check_connectivity(connectivity)
    marker, mask = _channel(marker, channel, 'the marker'), _channel(mask, mask_channel, 'the mask')
    if marker.shape != mask.shape:
        raise ValueError('the volumes differ in size: %r and %r' % (marker.shape, mask.shape))
    if marker.dtype != mask.dtype:
        raise ValueError('reconstruct needs volumes of one width, not %s and %s' % (marker.dtype, mask.dtype))
    return _reconstruct(marker, mask, code == RECONSTRUCT_OPS['erosion'], connectivity)


def geodesic_texels(array, op, h=0, connectivity=6, channel=0):
    """the texels vpt_volume_geodesic gives for ``array`` (module docstring): a [depth][height][width] array of its type"""
    check_geodesic_op(op)
    check_connectivity(connectivity)
    src = _channel(array, channel, 'the volume')
    largest = int(np.iinfo(src.dtype).max)
    h = check_h(op, h, largest)
    wide = src.astype(np.int64)
    if op in ('fill_holes', 'clear_border'):
        faces = np.zeros(src.shape, dtype=bool)
        faces[0], faces[-1], faces[:, 0], faces[:, -1], faces[:, :, 0], faces[:, :, -1] = (True,) * 6
        marker = np.where(faces, wide, largest if op == 'fill_holes' else 0).astype(src.dtype)
        r = _reconstruct(marker, src, op == 'fill_holes', connectivity)
        return r if op == 'fill_holes' else src - r
    if op in ('hmax', 'dome', 'maxima'):
        r = _reconstruct(np.maximum(wide - (1 if op == 'maxima' else h), 0).astype(src.dtype), src, False, connectivity)
        if op == 'hmax':
            return r
        return src - r if op == 'dome' else np.where(src > r, largest, 0).astype(src.dtype)
    r = _reconstruct(np.minimum(wide + (1 if op == 'minima' else h), largest).astype(src.dtype), src, True, connectivity)
    return r if op == 'hmin' else np.where(src < r, largest, 0).astype(src.dtype)
