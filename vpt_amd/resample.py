"""A volume resampled to any grid size, on the host: the numpy statement of the contract the device kernels (vpt_volume_resample;
include/vpt.h) are held to, for callers without a device and as the contract's documentation.

[depth][height][width] arrays, or [depth][height][width][2] for two channels; the target ``shape`` is (depth, height, width).  The cube the
volume occupies does not change, only the grid inside it.  n is a source axis length, N the matching target length, X a result index; every
division is a floor division of non-negative integers.

  nearest:   source index j = ((2 X + 1) n) // (2 N) per axis: the texel whose cell holds the centre of result texel X; its bits are copied.
             uint8, uint16, int8, int16 and float32 arrays.  The mode for label and mask volumes.
  filtered:  uint8 and uint16 arrays, per channel.  Each axis has non-negative integer tap weights with a constant sum S_axis:
               N >= n: linear interpolation at u = (X + 0.5) n / N - 0.5, clamped to the edge: num = (2 X + 1) n - N, D = 2 N;
                       num <= 0: (0, D); num >= (n - 1) D: (n - 1, D); else i = num // D, f = num % D: (i, D - f), (i + 1, f).  S_axis = 2 N.
               N <  n: the area average: w_j = min((X + 1) n, (j + 1) N) - max(X n, j N) for j = (X n) // N .. ((X + 1) n - 1) // N.  S_axis = n.
             With S = S_x S_y S_z and SUM the sum over all taps of w_x w_y w_z code:  out = (2 SUM + S) // (2 S), one rounding, halves up.
             2 SUM + S < 2^57: int64 holds everything, and the exact sum is taken axis by axis.

isotropic_shape gives the target size for cubic voxels from a spacing."""
import math

import numpy as np

MODES = {'nearest': 0, 'filtered': 1}
MAX_AXIS = 4096
_AXES = ('x', 'y', 'z')
_NEAREST_TYPES = (np.uint8, np.uint16, np.int8, np.int16, np.float32)


def check_mode(mode):
    """the code of 'nearest' (0: VPT_RESAMPLE_NEAREST) or 'filtered' (1: VPT_RESAMPLE_FILTERED); raises ValueError otherwise"""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("resample mode is 'filtered' or 'nearest', not %r" % (mode,))
    return MODES[mode]


def check_size(width, height, depth):
    """(width, height, depth) of a target grid: integers in 1 .. 4096; raises ValueError naming the axis otherwise"""
    out = []
    for axis, n in zip(_AXES, (width, height, depth)):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_AXIS:
            raise ValueError('resample size along %s is an integer in 1 .. %d, not %r' % (axis, MAX_AXIS, n))
        out.append(int(n))
    return tuple(out)


def _positive(value, what):
    if isinstance(value, (bool, str)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError('%s is a number, not %r' % (what, value))
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError('%s is finite and positive, not %r' % (what, value))
    return value


def check_spacing(spacing, pitch=None):
    """((sx, sy, sz), pitch) as floats: three finite spacings > 0 and a finite pitch > 0 (None: the smallest spacing); raises ValueError
    naming the axis otherwise"""
    if isinstance(spacing, (str, bytes)) or not hasattr(spacing, '__len__') or len(spacing) != 3:
        raise ValueError('spacing is (sx, sy, sz), not %r' % (spacing,))
    spacing = tuple(_positive(s, 'the spacing along %s' % axis) for axis, s in zip(_AXES, spacing))
    pitch = min(spacing) if pitch is None else _positive(pitch, 'pitch')
    return spacing, pitch


def isotropic_shape(size, spacing, pitch=None):
    """(Nx, Ny, Nz): the grid of cubic voxels of edge ``pitch`` (None: the smallest spacing) that fills the cube of a volume of ``size`` =
    (nx, ny, nz) voxels of ``spacing`` = (sx, sy, sz): N = max(1, floor(n * s / pitch + 0.5)) per axis, IEEE doubles in this order (one
    multiply, one divide, one add, floor).  Raises ValueError naming the axis when a spacing is not finite and positive or an N exceeds 4096."""
    if isinstance(size, (str, bytes)) or not hasattr(size, '__len__') or len(size) != 3:
        raise ValueError('size is (nx, ny, nz), not %r' % (size,))
    for axis, n in zip(_AXES, size):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= MAX_AXIS:
            raise ValueError('a volume has 1 .. %d voxels along %s, not %r' % (MAX_AXIS, axis, n))
    spacing, pitch = check_spacing(spacing, pitch)
    out = []
    for axis, n, s in zip(_AXES, size, spacing):
        cells = math.floor(float(n) * s / pitch + 0.5)
        if not cells <= MAX_AXIS:
            raise ValueError('the isotropic grid has %r voxels along %s: at most %d are taken (choose a larger pitch)' % (cells, axis, MAX_AXIS))
        out.append(max(1, int(cells)))
    return tuple(out)


def _axis(n, N):
    for what, v in (('source', n), ('target', N)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= MAX_AXIS:
            raise ValueError('a %s axis has 1 .. %d texels, not %r' % (what, MAX_AXIS, v))
    return int(n), int(N)


def nearest_index(n, N):
    """int64 [N]: the source index ((2 X + 1) n) // (2 N) of every result index X"""
    n, N = _axis(n, N)
    X = np.arange(N, dtype=np.int64)
    return ((2 * X + 1) * n) // (2 * N)


def axis_taps(n, N):
    """(taps, S): taps[X] = [(source index, weight), ...] of result index X with positive integer weights that sum to S (2 N where the
    axis grows or stays, n where it shrinks)"""
    n, N = _axis(n, N)
    taps = []
    if N >= n:
        D = 2 * N
        for X in range(N):
            num = (2 * X + 1) * n - N
            if num <= 0:
                taps.append([(0, D)])
            elif num >= (n - 1) * D:
                taps.append([(n - 1, D)])
            else:
                i, f = divmod(num, D)
                taps.append([(i, D - f), (i + 1, f)] if f else [(i, D)])
        return taps, D
    for X in range(N):
        taps.append([(j, min((X + 1) * n, (j + 1) * N) - max(X * n, j * N)) for j in range((X * n) // N, ((X + 1) * n - 1) // N + 1)])
    return taps, n


def _weights(n, N):
    """(int64 [N][n] weight matrix, S)"""
    taps, S = axis_taps(n, N)
    w = np.zeros((N, n), dtype=np.int64)
    for X, row in enumerate(taps):
        for j, weight in row:
            w[X, j] = weight
    return w, S


def _checked(array, shape, types, what):
    array = np.asarray(array)
    if array.ndim not in (3, 4) or (array.ndim == 4 and array.shape[3] != 2) or 0 in array.shape:
        raise ValueError('a volume is resampled from a [depth][height][width] or [depth][height][width][2] array')
    if array.dtype.type not in types:
        raise ValueError('%s resampling takes %s texels, not %s' % (what, ', '.join(np.dtype(t).name for t in types), array.dtype))
    if not hasattr(shape, '__len__') or len(shape) != 3:
        raise ValueError('the target shape is (depth, height, width), not %r' % (shape,))
    depth, height, width = shape
    width, height, depth = check_size(width, height, depth)
    if max(array.shape[:3]) > MAX_AXIS:
        raise ValueError('a volume has at most %d texels an axis' % MAX_AXIS)
    return array, (depth, height, width)


def _sums(array, shape):
    """(int64 sums over all taps, S) of a checked uint8 / uint16 array"""
    v = array.astype(np.int64)
    S = 1
    for axis in (2, 1, 0):                                        # x, y, z: the sum is exact, the order changes nothing
        w, s = _weights(array.shape[axis], shape[axis])
        v = np.moveaxis(np.tensordot(w, v, axes=([1], [axis])), 0, axis)
        S *= s
    return v, S


def resample_texels(array, shape, mode='filtered'):
    """The array on the grid ``shape`` = (depth, height, width), in the array's dtype: what ``Volume.resample(width, height, depth, mode)``
    holds on the device, byte for byte."""
    if check_mode(mode) == 0:
        array, shape = _checked(array, shape, _NEAREST_TYPES, 'nearest')
        iz, iy, ix = (nearest_index(n, N) for n, N in zip(array.shape[:3], shape))
        return np.ascontiguousarray(array[iz][:, iy][:, :, ix])
    array, shape = _checked(array, shape, (np.uint8, np.uint16), 'filtered')
    v, S = _sums(array, shape)
    return np.ascontiguousarray((2 * v + S) // (2 * S)).astype(array.dtype)


def count_ties(array, shape):
    """the number of result texels (per channel) of the filtered resampling whose exact value lies halfway between two codes: where the
    rounding rule (halves up) decides"""
    array, shape = _checked(array, shape, (np.uint8, np.uint16), 'filtered')
    v, S = _sums(array, shape)
    return int(np.count_nonzero((2 * v) % (2 * S) == S))
