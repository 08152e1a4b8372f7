"""Volume — src/js/Volume.js:3-127 re-hosted on HIP device memory; driven by a reader (vpt_amd/readers.py) the way
RenderingContext.setVolume does (RenderingContext.js:124-134)."""
import ctypes as C

import numpy as np

from . import _native as N
from .property_bag import EventTarget, CustomEvent

from .readers import (RAWReader, GL_RED, GL_R8, GL_RG, GL_RG8, GL_UNSIGNED_BYTE, GL_RGB, GL_RGB8, GL_RGBA, GL_RGBA8,      # noqa: F401  (re-exported)
                      GL_FLOAT, GL_HALF_FLOAT, GL_R32F, GL_R16F,
                      GL_BYTE, GL_R8_SNORM, GL_RG8_SNORM, GL_RGB8_SNORM, GL_RGBA8_SNORM,
                      GL_UNSIGNED_SHORT_5_6_5, GL_RGB565, GL_UNSIGNED_SHORT_4_4_4_4, GL_RGBA4, GL_UNSIGNED_SHORT_5_5_5_1, GL_RGB5_A1,
                      GL_UNSIGNED_INT_2_10_10_10_REV, GL_RGB10_A2, GL_UNSIGNED_INT_10F_11F_11F_REV, GL_R11F_G11F_B10F,
                      GL_UNSIGNED_INT_5_9_9_9_REV, GL_RGB9_E5,
                      GL_UNSIGNED_SHORT, GL_SHORT, GL_R16_EXT, GL_RG16_EXT, GL_RGB16_EXT, GL_RGBA16_EXT,
                      GL_R16_SNORM_EXT, GL_RG16_SNORM_EXT, GL_RGB16_SNORM_EXT, GL_RGBA16_SNORM_EXT)

# (type, format, internalFormat) -> (native format, channels in the file, numpy dtype of a block) for the formats keyed on all three:
# SNORM bytes (RGB8_SNORM / RGBA8_SNORM keep their first two channels, as RGB8 / RGBA8 do) and the packed types, one word per texel
_SIZED = {
    (GL_BYTE, GL_RED, GL_R8_SNORM): ('FORMAT_R8_SNORM', 1, np.int8),
    (GL_BYTE, GL_RG, GL_RG8_SNORM): ('FORMAT_RG8_SNORM', 2, np.int8),
    (GL_BYTE, GL_RGB, GL_RGB8_SNORM): ('FORMAT_RG8_SNORM', 3, np.int8),
    (GL_BYTE, GL_RGBA, GL_RGBA8_SNORM): ('FORMAT_RG8_SNORM', 4, np.int8),
    (GL_UNSIGNED_SHORT_5_6_5, GL_RGB, GL_RGB565): ('FORMAT_RGB565', 1, np.uint16),
    (GL_UNSIGNED_SHORT_4_4_4_4, GL_RGBA, GL_RGBA4): ('FORMAT_RGBA4', 1, np.uint16),
    (GL_UNSIGNED_SHORT_5_5_5_1, GL_RGBA, GL_RGB5_A1): ('FORMAT_RGB5_A1', 1, np.uint16),
    (GL_UNSIGNED_INT_2_10_10_10_REV, GL_RGBA, GL_RGB10_A2): ('FORMAT_RGB10_A2', 1, np.uint32),
    (GL_UNSIGNED_INT_10F_11F_11F_REV, GL_RGB, GL_R11F_G11F_B10F): ('FORMAT_R11F_G11F_B10F', 1, np.uint32),
    (GL_UNSIGNED_INT_5_9_9_9_REV, GL_RGB, GL_RGB9_E5): ('FORMAT_RGB9_E5', 1, np.uint32),
}
# ... and those a context takes once it has enabled EXT_texture_norm16 (gl.getExtension): 16-bit normalised channels, uploaded as they are
# (RGB16 / RGBA16 keep their first two channels)
_NORM16 = {
    (GL_UNSIGNED_SHORT, GL_RED, GL_R16_EXT): ('FORMAT_R16', 1, np.uint16),
    (GL_UNSIGNED_SHORT, GL_RG, GL_RG16_EXT): ('FORMAT_RG16', 2, np.uint16),
    (GL_UNSIGNED_SHORT, GL_RGB, GL_RGB16_EXT): ('FORMAT_RG16', 3, np.uint16),
    (GL_UNSIGNED_SHORT, GL_RGBA, GL_RGBA16_EXT): ('FORMAT_RG16', 4, np.uint16),
    (GL_SHORT, GL_RED, GL_R16_SNORM_EXT): ('FORMAT_R16_SNORM', 1, np.int16),
    (GL_SHORT, GL_RG, GL_RG16_SNORM_EXT): ('FORMAT_RG16_SNORM', 2, np.int16),
    (GL_SHORT, GL_RGB, GL_RGB16_SNORM_EXT): ('FORMAT_RG16_SNORM', 3, np.int16),
    (GL_SHORT, GL_RGBA, GL_RGBA16_SNORM_EXT): ('FORMAT_RG16_SNORM', 4, np.int16),
}
NORM16_EXTENSION = 'EXT_texture_norm16'


def device_format(modality, gl=None):
    """(native format, channels in the file, numpy dtype of a block) for a manifest's (type, format, internalFormat) — Volume.js:58-60
    allocates whatever internalFormat the manifest names and :84-105 `_typize` maps the GL type to a typed array.  What a WebGL2
    sampler3D can filter is what is taken here: UNSIGNED_BYTE and FLOAT / HALF_FLOAT (half widens to float exactly) with 1-4 channels —
    the shaders read .rg, so channels past the second are dropped on upload (R8, RG8; R32F, RG32F) —; BYTE with an SNORM internal format
    (R8_SNORM, RG8_SNORM; RGB8_SNORM / RGBA8_SNORM keep two channels); and the packed types with the one internal format each names
    (RGB565, RGBA4, RGB5_A1, RGB10_A2, R11F_G11F_B10F, RGB9_E5: uploaded as words, decoded on the device).  Integer textures need a
    usampler3D / isampler3D, 16-bit normalised ones an extension the reference does not enable, and 3-D depth textures do not exist in
    ES 3.0: every other combination raises the reference's error.  ``gl``: the volume's context; once it has enabled EXT_texture_norm16
    (gl.getExtension), UNSIGNED_SHORT / SHORT with that extension's R16 / RG16 / RGB16 / RGBA16 (_SNORM) internal formats are taken too."""
    t, f = modality['type'], modality['format']
    if t == GL_UNSIGNED_BYTE and f in (GL_RED, GL_RG, GL_RGB, GL_RGBA):
        n = {GL_RED: 1, GL_RG: 2, GL_RGB: 3, GL_RGBA: 4}[f]
        return (N.FORMAT_R8 if n == 1 else N.FORMAT_RG8), n, np.uint8
    if t in (GL_FLOAT, GL_HALF_FLOAT) and f in (GL_RED, GL_RG, GL_RGB, GL_RGBA):
        n = {GL_RED: 1, GL_RG: 2, GL_RGB: 3, GL_RGBA: 4}[f]
        return (N.FORMAT_R32F if n == 1 else N.FORMAT_RG32F), n, (np.float32 if t == GL_FLOAT else np.float16)
    sized = _SIZED.get((t, f, modality.get('internalFormat')))
    if sized is None and gl is not None and gl.extension_enabled(NORM16_EXTENSION):
        sized = _NORM16.get((t, f, modality.get('internalFormat')))
    if sized is not None:
        return getattr(N, sized[0]), sized[1], sized[2]
    raise RuntimeError('Unknown volume datatype: %s' % t)                   # Volume.js:103



def filter_code(filter):
    """The VPT_FILTER_* code of a setFilter() name: 'linear', 'quasicubic' (smoothstep-weighted LINEAR cell, C1), and anything else
    'nearest' (Volume.js:121)."""
    if filter == 'linear':
        return N.FILTER_LINEAR
    if filter == 'quasicubic':
        return N.FILTER_QUASI_CUBIC
    return N.FILTER_NEAREST

def _derived_volume(out, handle, modality, meta, dims):
    """``out``, a new Volume, made ready around the derived native volume ``handle``: ``modality`` with the dimensions ``dims`` in one
    block, and a copy of ``meta``"""
    out.texture = handle
    out.modality = dict(modality, dimensions=dict(dims), placements=[{'index': 0, 'position': {'x': 0, 'y': 0, 'z': 0}}])
    out.metadata = {'meta': dict(meta), 'modalities': [out.modality],
                    'blocks': [{'url': None, 'format': 'raw', 'dimensions': dict(dims)}]}
    out.ready = True
    return out


class Volume(EventTarget):
    """Volume.js:3-127.  ``gl`` is a vpt_amd.Context.  ``getTexture()`` returns the native volume handle
    once ``ready`` (the reference returns the WebGLTexture), else None."""

    def __init__(self, gl, reader=None, options=None):
        super().__init__()
        self._gl = gl
        self._reader = reader
        self.metadata = None
        self.ready = False
        self.texture = None
        self.modality = None

    def destroy(self):
        if self.texture:
            N.lib().vpt_volume_destroy(self.texture)
            self.texture = None
            self.ready = False

    def readMetadata(self):
        if not self.metadata:
            self.metadata = self._reader.readMetadata()
        return self.metadata

    def readModality(self, modalityName):
        L = N.lib()
        self.ready = False
        if not self.metadata:
            self.readMetadata()
        modality = next((m for m in self.metadata['modalities'] if m['name'] == modalityName), None)
        if modality is None:
            raise RuntimeError("Modality '%s' does not exist" % modalityName)      # Volume.js:40
        self.modality = modality
        if self.texture:
            L.vpt_volume_destroy(self.texture)
            self.texture = None
        dims = modality['dimensions']
        fmt, nch, dtype = device_format(modality, self._gl)
        h = C.c_void_p()
        N.check(L.vpt_volume_create(self._gl._h, dims['width'], dims['height'], dims['depth'], fmt, C.byref(h)))
        self.texture = h
        placements = modality['placements']
        for placement in placements:
            index, position = placement['index'], placement['position']
            raw = self._reader.readBlock(index)
            bd = self.metadata['blocks'][index]['dimensions']
            data = np.frombuffer(raw, dtype=dtype) if isinstance(raw, (bytes, bytearray, memoryview)) else np.asarray(raw).view(dtype).reshape(-1)
            if nch > 2:                                   # RGB8 / RGBA8: texture(uVolume, p).rg reads the first two channels
                data = data.reshape(-1, nch)[:, :2]
            if dtype in (np.float16, np.float32):
                data = data.astype(np.float32)            # HALF_FLOAT widens exactly
            data = np.ascontiguousarray(data)
            N.check(L.vpt_volume_upload_block(self.texture, position['x'], position['y'], position['z'],
                                              bd['width'], bd['height'], bd['depth'],
                                              data.ctypes.data_as(C.c_void_p), data.nbytes))
            progress = (index + 1) / len(placements)
            self.dispatchEvent(CustomEvent('progress', {'detail': progress}))
        N.check(L.vpt_volume_finalize(self.texture))
        self.ready = True

    def load(self):
        self.readModality('default')

    def getTexture(self):
        return self.texture if self.ready else None

    def setFilter(self, filter):
        if not self.texture:
            return
        N.check(N.lib().vpt_volume_set_filter(self.texture, filter_code(filter)))

    # ---- extension: whole-array upload (one block) for synthetic volumes ----
    @classmethod
    def from_array(cls, gl, array, filter='linear', snorm=False, norm16=False):
        """Upload a [depth][height][width] (uint8: R8; float16 / float32: R32F) or [depth][height][width][2] (RG8 / RG32F) array (host -> HBM once).
        ``snorm=True``: the array is int8 and becomes an R8_SNORM / RG8_SNORM volume (texel c reads as max(c / 127, -1)).
        ``norm16=True``: the array is uint16 (R16 / RG16: c reads as c / 65535) or int16 (R16_SNORM / RG16_SNORM: max(c / 32767, -1)),
        kept at 2 bytes per channel (EXT_texture_norm16)."""
        array = np.asarray(array)
        if snorm:
            if array.dtype != np.int8:
                raise ValueError('an SNORM volume is uploaded from an int8 array')
            return cls._from_raw_array(gl, array, filter, (N.FORMAT_R8_SNORM, N.FORMAT_RG8_SNORM), GL_BYTE, (GL_R8_SNORM, GL_RG8_SNORM))
        if norm16:
            if array.dtype == np.uint16:
                return cls._from_raw_array(gl, array, filter, (N.FORMAT_R16, N.FORMAT_RG16), GL_UNSIGNED_SHORT, (GL_R16_EXT, GL_RG16_EXT))
            if array.dtype == np.int16:
                return cls._from_raw_array(gl, array, filter, (N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM), GL_SHORT,
                                           (GL_R16_SNORM_EXT, GL_RG16_SNORM_EXT))
            raise ValueError('a 16-bit normalised volume is uploaded from a uint16 (UNORM) or int16 (SNORM) array')
        f32 = array.dtype.kind == 'f'
        array = np.ascontiguousarray(array, dtype=np.float32 if f32 else np.uint8)
        if array.ndim == 4 and array.shape[3] != 2:
            raise ValueError('a two-channel volume is [depth][height][width][2]')
        d, h, w = array.shape[:3]
        channels = 2 if array.ndim == 4 else 1
        vox = channels * (4 if f32 else 1)
        vol = cls(gl, RAWReader(array.view(np.uint8), {'width': w * vox, 'height': h, 'depth': d}))      # slices of w * vox bytes
        L = N.lib()
        hnd = C.c_void_p()
        fmt = (N.FORMAT_RG32F if channels == 2 else N.FORMAT_R32F) if f32 else (N.FORMAT_RG8 if channels == 2 else N.FORMAT_R8)
        N.check(L.vpt_volume_create(gl._h, w, h, d, fmt, C.byref(hnd)))
        vol.texture = hnd
        # chunk along z so one call stays < 2 GiB
        zs = max(1, (1 << 30) // (w * h * vox))
        for z0 in range(0, d, zs):
            z1 = min(d, z0 + zs)
            chunk = array[z0:z1]
            N.check(L.vpt_volume_upload_block(hnd, 0, 0, z0, w, h, z1 - z0, chunk.ctypes.data_as(C.c_void_p), chunk.nbytes))
        N.check(L.vpt_volume_finalize(hnd))
        vol.metadata = vol._reader.readMetadata()
        vol.modality = vol.metadata['modalities'][0]
        if vox > 1:                                         # the slices were handed over as w * vox bytes wide: restore the description
            vol.modality['dimensions']['width'] = w
            if f32 and channels == 2:
                vol.modality['format'], vol.modality['internalFormat'], vol.modality['type'] = GL_RG, 0x8230, GL_FLOAT      # RG32F
            elif f32:
                vol.modality['format'], vol.modality['internalFormat'], vol.modality['type'] = GL_RED, GL_R32F, GL_FLOAT
            else:
                vol.modality['format'], vol.modality['internalFormat'] = GL_RG, GL_RG8
            for b in vol.metadata['blocks']:
                b['dimensions']['width'] = w
        vol.ready = True
        vol.setFilter(filter)
        return vol

    @classmethod
    def _from_raw_array(cls, gl, array, filter, formats, gltype, internal_formats):
        """the texels uploaded as they are: formats / internal_formats = (one channel, two channels)"""
        array = np.ascontiguousarray(array)
        if array.ndim == 4 and array.shape[3] != 2:
            raise ValueError('a two-channel volume is [depth][height][width][2]')
        d, h, w = array.shape[:3]
        channels = 2 if array.ndim == 4 else 1
        vox = channels * array.dtype.itemsize
        vol = cls(gl, RAWReader(array.view(np.uint8), {'width': w * vox, 'height': h, 'depth': d}))
        L = N.lib()
        hnd = C.c_void_p()
        N.check(L.vpt_volume_create(gl._h, w, h, d, formats[channels - 1], C.byref(hnd)))
        vol.texture = hnd
        zs = max(1, (1 << 30) // (w * h * vox))
        for z0 in range(0, d, zs):
            chunk = array[z0:min(d, z0 + zs)]
            N.check(L.vpt_volume_upload_block(hnd, 0, 0, z0, w, h, chunk.shape[0], chunk.ctypes.data_as(C.c_void_p), chunk.nbytes))
        N.check(L.vpt_volume_finalize(hnd))
        vol.metadata = vol._reader.readMetadata()
        vol.modality = vol.metadata['modalities'][0]
        vol.modality['dimensions']['width'] = w
        vol.modality['type'] = gltype
        vol.modality['format'], vol.modality['internalFormat'] = (GL_RG if channels == 2 else GL_RED), internal_formats[channels - 1]
        for b in vol.metadata['blocks']:
            b['dimensions']['width'] = w
        vol.ready = True
        vol.setFilter(filter)
        return vol

    def upload_block(self, x, y, z, block):
        """(extension) texSubImage3D of one more block into the ready volume: `block` is [depth][height][width] in the volume's texel type;
        the device layouts are rebuilt by the next pass that samples the volume"""
        block = np.ascontiguousarray(block)
        d, h, w = block.shape[:3]
        N.check(N.lib().vpt_volume_upload_block(self.texture, int(x), int(y), int(z), w, h, d, block.ctypes.data_as(C.c_void_p), block.nbytes))

    def upload_block_device(self, x, y, z, w, h, d, device_ptr, nbytes):
        """(extension) the same from memory already in HBM on the context's device (e.g. a torch tensor's data_ptr())"""
        N.check(N.lib().vpt_volume_upload_block_device(self.texture, int(x), int(y), int(z), int(w), int(h), int(d),
                                                       C.c_void_p(int(device_ptr)), int(nbytes)))

    # ---- extension: volume operations on the device (include/vpt.h; DESIGN.md "Gradient-magnitude channel") ----
    def native_format(self):
        """(VPT_FORMAT_* of the device volume, numpy dtype of a block's texels) from the modality (a 16-bit volume made by from_array
        needs no extension: its triple is looked up directly)"""
        m = self.modality
        key = (m['type'], m['format'], m.get('internalFormat'))
        sized = _SIZED.get(key) or _NORM16.get(key)
        if sized is not None:
            return getattr(N, sized[0]), sized[2]
        fmt, _, dtype = device_format(m, self._gl)
        return fmt, dtype

    def _texel_layout(self):
        """(channels, numpy dtype) of a block as upload_block takes it and read_block returns it (packed formats: the decoded RG32F texels)"""
        fmt, dtype = self.native_format()
        if fmt in (N.FORMAT_R32F, N.FORMAT_RG32F):
            dtype = np.float32                                # HALF_FLOAT was widened on upload
        if N.FORMAT_RGB565 <= fmt <= N.FORMAT_RGB9_E5:
            return 2, np.float32
        two = fmt in (N.FORMAT_RG8, N.FORMAT_RG32F, N.FORMAT_RG8_SNORM, N.FORMAT_RG16, N.FORMAT_RG16_SNORM)
        return (2 if two else 1), dtype

    def read_block(self, x, y, z, w, h, d):
        """texSubImage3D's inverse: the texels of a box as a [d][h][w] (one channel) or [d][h][w][2] array in the volume's texel type"""
        channels, dtype = self._texel_layout()
        out = np.empty((int(d), int(h), int(w)) + ((2,) if channels == 2 else ()), dtype=dtype)
        N.check(N.lib().vpt_volume_read_block(self.texture, int(x), int(y), int(z), int(w), int(h), int(d),
                                              out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def histogram(self):
        """uint32 counts: [256] bins of the value's top 8 bits (R8 / R16), or [256][256], [g][v], of both channels' (RG8 / RG16).  A volume
        of more than 2^32 - 1 voxels raises VptError (ERR_UNSUPPORTED): the bins are 32-bit."""
        channels, _ = self._texel_layout()
        bins = np.zeros(65536 if channels == 2 else 256, dtype=np.uint32)
        N.check(N.lib().vpt_volume_histogram(self.texture, bins.ctypes.data_as(C.POINTER(C.c_uint32)), bins.size))
        return bins.reshape(256, 256) if channels == 2 else bins

    def derive_gradient(self, operator='central', gain=1.0):
        """A new, ready RG8 / RG16 volume on this volume's context and with its filter: channel 0 this (R8 / R16) volume's texels, channel 1
        their gradient magnitude (vpt_amd.gradient_magnitude states it), derived on the device.  This volume is not changed."""
        from .gradient import operator_code, gain_factor
        op = operator_code(operator)
        gain_factor(gain)                                     # raises for gains the contract does not take
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_derive_gradient(self.texture, op, float(gain), C.byref(h)))
        out = type(self)(self._gl)
        out.texture = h
        norm16 = self.modality.get('internalFormat') == GL_R16_EXT
        dims = dict(self.modality['dimensions'])
        out.modality = {'name': self.modality.get('name', 'default'), 'dimensions': dims, 'transform': self.modality.get('transform'),
                        'format': GL_RG, 'internalFormat': GL_RG16_EXT if norm16 else GL_RG8,
                        'type': GL_UNSIGNED_SHORT if norm16 else GL_UNSIGNED_BYTE,
                        'placements': [{'index': 0, 'position': {'x': 0, 'y': 0, 'z': 0}}]}
        out.metadata = {'meta': dict((self.metadata or {}).get('meta', {})), 'modalities': [out.modality],
                        'blocks': [{'url': None, 'format': 'raw', 'dimensions': dict(dims)}]}
        out.ready = True
        return out

    # ---- extension: the value-range window (include/vpt.h; DESIGN.md "Value-range window") ----
    def window(self, lo, hi, format='r8'):
        """A new, ready R8 / R16 volume on this volume's context and with its filter whose [0, 1] axis is the value range [lo, hi] of
        this one-channel volume (code units for R8 / R16 / R8_SNORM / R16_SNORM, values for R32F): 0 at or below lo, the largest texel at or
        above hi (vpt_amd.window_texels states it), derived on the device.  This volume is not changed."""
        from .window import format_bits
        norm16 = format_bits(format) == 16
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_window(self.texture, float(lo), float(hi), N.FORMAT_R16 if norm16 else N.FORMAT_R8, C.byref(h)))
        out = type(self)(self._gl)
        out.texture = h
        dims = dict(self.modality['dimensions'])
        out.modality = {'name': self.modality.get('name', 'default'), 'dimensions': dims, 'transform': self.modality.get('transform'),
                        'format': GL_RED, 'internalFormat': GL_R16_EXT if norm16 else GL_R8,
                        'type': GL_UNSIGNED_SHORT if norm16 else GL_UNSIGNED_BYTE,
                        'placements': [{'index': 0, 'position': {'x': 0, 'y': 0, 'z': 0}}]}
        out.metadata = {'meta': dict((self.metadata or {}).get('meta', {})), 'modalities': [out.modality],
                        'blocks': [{'url': None, 'format': 'raw', 'dimensions': dict(dims)}]}
        out.ready = True
        return out

    def range(self):
        """(lo, hi): the smallest and the largest code (ints; R8 / R16 / R8_SNORM / R16_SNORM) or value (floats; R32F, NaN texels ignored)"""
        lo, hi = C.c_double(0), C.c_double(0)
        N.check(N.lib().vpt_volume_range(self.texture, C.byref(lo), C.byref(hi)))
        if self.native_format()[0] == N.FORMAT_R32F:
            return lo.value, hi.value
        return int(lo.value), int(hi.value)

    def code_histogram(self):
        """uint32 counts per code at full resolution: [256] (R8, R8_SNORM) or [65536] (R16, R16_SNORM) bins; bin = code, for SNORM
        code + 128 / code + 32768.  A volume of more than 2^32 - 1 voxels raises VptError (ERR_UNSUPPORTED): the bins are 32-bit; so do
        ``percentile_window`` and a RenderingContext whose window is given in percentiles."""
        fmt = self.native_format()[0]
        bins = np.zeros(65536 if fmt in (N.FORMAT_R16, N.FORMAT_R16_SNORM) else 256, dtype=np.uint32)
        N.check(N.lib().vpt_volume_code_histogram(self.texture, bins.ctypes.data_as(C.POINTER(C.c_uint32)), bins.size))
        return bins

    def percentile_window(self, p_lo=0.5, p_hi=99.5):
        """(lo, hi) in code units: the p_lo-th and p_hi-th percentile codes of an integer volume (vpt_amd.percentile_window)"""
        from .window import percentile_window
        signed = self.native_format()[0] in (N.FORMAT_R8_SNORM, N.FORMAT_R16_SNORM)
        return percentile_window(self.code_histogram(), p_lo, p_hi, signed)

    # ---- extension: the next coarser level and binomial smoothing (include/vpt.h; DESIGN.md "Binomial smoothing and 2x reduction") ----
    def _same_format(self, handle, dims):
        """the ready Volume around a derived native volume of this volume's format with the dimensions ``dims``"""
        return _derived_volume(type(self)(self._gl), handle, self.modality, (self.metadata or {}).get('meta', {}), dims)

    def reduce(self, levels=1):
        """A new, ready volume in this volume's format and with its filter, ``levels`` times reduced to ceil(n / 2) texels per axis: every
        texel the rounded mean of its 2 x 2 x 2 cell (vpt_amd.reduce_texels states it), derived on the device.  Stops early once every axis
        is 1 (the result is then a copy).  Packed formats are refused.  This volume is not changed."""
        from .pyramid import check_levels
        levels = check_levels(levels)
        L = N.lib()
        source, dims = self, dict(self.modality['dimensions'])
        while True:
            h = C.c_void_p()
            try:
                N.check(L.vpt_volume_reduce(source.texture, C.byref(h)))
            finally:
                if source is not self:
                    source.destroy()                          # the level in between
            dims = {k: (dims[k] + 1) // 2 for k in ('width', 'height', 'depth')}
            source = self._same_format(h, dims)
            levels -= 1
            if levels == 0 or max(dims.values()) == 1:
                return source

    def smooth(self, passes=1):
        """A new, ready R8 / R16 volume of this (R8 / R16) volume's size and with its filter: ``passes`` (1 .. 8) applications of the binomial
        3 x 3 x 3 kernel (vpt_amd.smooth_texels states it), derived on the device.  This volume is not changed."""
        from .pyramid import check_passes
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_smooth(self.texture, check_passes(passes), C.byref(h)))
        return self._same_format(h, self.modality['dimensions'])

    # ---- extension: median and grey-level morphology (include/vpt.h; DESIGN.md "Median and morphology") ----
    def rank(self, op, passes=1):
        """A new, ready R8 / R16 volume of this (R8 / R16) volume's size and with its filter: ``passes`` (1 .. 8) applications of the rank
        operator ``op`` ('median' | 'erode' | 'dilate' | 'open' | 'close') over the clamped 3 x 3 x 3 box (vpt_amd.rank_texels states it),
        derived on the device.  This volume is not changed."""
        from .rank import operator_code, check_passes
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_rank(self.texture, operator_code(op), check_passes(passes), C.byref(h)))
        return self._same_format(h, self.modality['dimensions'])

    def median(self, passes=1):
        return self.rank('median', passes)

    def erode(self, passes=1):
        return self.rank('erode', passes)

    def dilate(self, passes=1):
        return self.rank('dilate', passes)

    def open(self, passes=1):
        return self.rank('open', passes)

    def close(self, passes=1):
        return self.rank('close', passes)

    # ---- extension: connected components of a value range (include/vpt.h; DESIGN.md "Connected components") ----
    def components(self, lo, hi, connectivity=6, min_voxels=1, _caps=None):
        """The connected components of the codes lo .. hi of this (R8 / R16) volume as a ``Components`` object, labelled on the device
        (vpt_amd.components_texels states the contract).  The object owns what it needs: this volume is not changed and may be destroyed.
        ``_caps`` (for tests): (merge_steps, flatten_steps) of vpt_volume_components_capped."""
        from .components import check_connectivity, check_min_voxels, check_range
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        connectivity, min_voxels = check_connectivity(connectivity), check_min_voxels(min_voxels)
        h = C.c_void_p()
        if _caps is None:
            N.check(N.lib().vpt_volume_components(self.texture, lo, hi, connectivity, min_voxels, C.byref(h)))
        else:
            merge_steps, flatten_steps = _caps
            N.check(N.lib().vpt_volume_components_capped(self.texture, lo, hi, connectivity, min_voxels, int(merge_steps), int(flatten_steps), C.byref(h)))
        return Components(self, h)

    def keep_largest(self, lo, hi, n=1, connectivity=6):
        """A new, ready volume like this one in which only the ``n`` largest components of the codes lo .. hi keep their codes; 0 elsewhere"""
        c = self.components(lo, hi, connectivity)
        try:
            return c.keep(1, n)
        finally:
            c.destroy()

    def remove_islands(self, lo, hi, min_voxels, connectivity=6):
        """A new, ready volume like this one in which the components of the codes lo .. hi with at least ``min_voxels`` voxels keep their
        codes; 0 elsewhere"""
        c = self.components(lo, hi, connectivity, min_voxels)
        try:
            return c.keep(1, None)
        finally:
            c.destroy()

    # ---- extension: exact Euclidean distance transform of a value range (include/vpt.h; DESIGN.md "Distance transform") ----
    def distance(self, lo, hi, seeds='range'):
        """The squared Euclidean distance of every voxel of this (R8 / R16) volume to the nearest voxel whose code is (seeds 'range') or is
        not (seeds 'rest') in lo .. hi, as a ``Distance`` object, transformed on the device (vpt_amd.distance_squared_texels states the
        contract).  The object owns what it needs: this volume is not changed and may be destroyed."""
        from .distance import check_range, check_seeds
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_distance(self.texture, lo, hi, check_seeds(seeds), C.byref(h)))
        return Distance(self, h)

    def margin(self, lo, hi, radius):
        """A new, ready volume like this one that keeps its codes within ``radius`` voxels of the codes lo .. hi; 0 elsewhere"""
        from .distance import check_radius
        r2 = check_radius(radius)
        d = self.distance(lo, hi, 'range')
        try:
            return d.within(0, r2)
        finally:
            d.destroy()

    def core(self, lo, hi, radius):
        """A new, ready volume like this one in which the codes lo .. hi eroded by the Euclidean ball of ``radius`` voxels keep their
        codes (the voxels deeper than ``radius`` inside the structure); 0 elsewhere"""
        from .distance import check_radius
        r2 = check_radius(radius)
        d = self.distance(lo, hi, 'rest')
        try:
            return d.within(r2 + 1, None)
        finally:
            d.destroy()

    # ---- extension: local thickness, the largest inscribed ball (include/vpt.h; DESIGN.md "Local thickness") ----
    def _thickness(self, lo, hi, seeds, emit):
        d = self.distance(lo, hi, seeds)
        try:
            t = d.thickness()
        finally:
            d.destroy()
        try:
            return emit(t)
        finally:
            t.destroy()

    def thickness(self, lo, hi, steps=2, seeds='rest'):
        """A new, ready RG8 / RG16 volume (code, local thickness): the second channel is, in ``steps`` rows a voxel (2: the diameter in
        voxels), the radius of the largest ball that fits inside the structure of the codes lo .. hi (seeds 'rest'; 'range': inside its
        complement: pore size, separation) and holds the voxel: distance(lo, hi, seeds) -> thickness() -> channel(steps), all on the
        device (vpt_amd.thickness_texels states it).  A valid ``values`` argument of ``Components.measure``."""
        from .distance import check_steps
        steps = check_steps(steps)
        return self._thickness(lo, hi, seeds, lambda t: t.channel(steps))

    def open_ball(self, lo, hi, radius, fill=0):
        """A new, ready volume like this one in which the codes lo .. hi opened by the Euclidean ball of ``radius`` voxels keep their
        codes (the parts some inscribed ball of radius > ``radius`` covers), ``fill`` elsewhere (vpt_amd.open_ball_texels states it): the
        counterpart of ``core`` that gives the peeled rim back"""
        from .distance import check_radius
        r2 = check_radius(radius)
        return self._thickness(lo, hi, 'rest', lambda t: t.within(r2 + 1, None, fill))

    # ---- extension: curve skeleton and topological kernel by thinning (include/vpt.h; DESIGN.md "Skeleton") ----
    def skeleton(self, lo, hi, mode='ends', passes=0, _flags=None):
        """The burn passes of thinning the codes lo .. hi of this (R8 / R16) volume, as a ``Skeleton`` object, thinned on the device
        (vpt_amd.skeleton_burn_texels states the contract): mode 'kernel' shrinks every structure to its topological kernel (a ball to a
        voxel, a torus to a closed curve), 'ends' keeps curve ends (the centreline), 'isthmus' keeps the voxels that once held two parts
        together; ``passes`` caps the passes (0: to the fixed point).  The object owns what it needs: this volume is not changed and may
        be destroyed.  ``_flags`` (for tests): the flags of vpt_volume_skeleton_capped (1: no tile cull)."""
        from .skeleton import check_mode, check_passes, check_range
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        code, passes = check_mode(mode), check_passes(passes)
        h = C.c_void_p()
        if _flags is None:
            N.check(N.lib().vpt_volume_skeleton(self.texture, lo, hi, code, passes, C.byref(h)))
        else:
            N.check(N.lib().vpt_volume_skeleton_capped(self.texture, lo, hi, code, passes, int(_flags), C.byref(h)))
        return Skeleton(self, h)

    def centreline(self, lo, hi, mode='ends', prune=None, prune_rounds=1):
        """A new, ready volume like this one in which the voxels of the codes lo .. hi that survive the thinning keep their codes; 0
        elsewhere (vpt_amd.skeleton_texels states it).  With ``prune`` (a length in the default step weights 10 / 14 / 17: ten a voxel),
        up to ``prune_rounds`` times: the skeleton's graph, its spurs within ``prune`` dropped (``Graph.prune``), the rest thinned again;
        a round that drops nothing ends it (vpt_amd.graph.centreline_texels states it).  The pruned volume is filled with a code outside
        lo .. hi (0 when lo > 0, otherwise hi + 1), so a range that covers every code is refused with ``prune`` set."""
        if prune is None:
            k = self.skeleton(lo, hi, mode)
            try:
                return k.volume()
            finally:
                k.destroy()
        from .graph import check_centreline_prune, dropped
        from .skeleton import check_range
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        prune, prune_rounds, fill = check_centreline_prune(lo, hi, prune, prune_rounds, 65535 if norm16 else 255)
        k = self.skeleton(lo, hi, mode)
        try:
            for _ in range(prune_rounds):
                g = k.graph()
                try:
                    if not dropped(g.branch_records(), prune).any():
                        break
                    pruned = g.prune(prune, fill=fill)
                finally:
                    g.destroy()
                try:
                    again = pruned.skeleton(lo, hi, mode)
                finally:
                    pruned.destroy()
                k.destroy()
                k = again
            return k.volume()
        finally:
            k.destroy()

    # ---- extension: the graph of a voxel set: branches, nodes, step counts, spur pruning (include/vpt.h; DESIGN.md "Skeleton graph") ----
    def graph(self, lo, hi):
        """The graph of the voxels of the codes lo .. hi of this (R8 / R16) volume as a ``Graph`` object, built on the device
        (vpt_amd.graph.graph_texels states the contract): meant for a thinned set (``centreline``), defined for any.  The object owns what
        it needs: this volume is not changed and may be destroyed."""
        from .graph import check_range
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_graph(self.texture, lo, hi, C.byref(h)))
        return Graph(self, h)

    # ---- extension: isosurface mesh by naive surface nets (include/vpt.h; DESIGN.md "Surface") ----
    def surface(self, level, channel=0, _scan_words=None):
        """The surface at code ``level`` - 1/2 of channel ``channel`` of this (R8, RG8, R16 or RG16) volume as a ``Surface`` object: one
        vertex per cell the surface crosses, one quad per grid edge it crosses, extracted on the device (vpt_amd.surface.surface_texels
        states the contract).  The object owns what it holds: this volume is not changed and may be destroyed.  ``_scan_words`` (for
        tests): the words per block of the prefix sums of vpt_volume_surface_capped."""
        from .surface import check_channel, check_level
        fmt = self.native_format()[0]
        norm16 = fmt in (N.FORMAT_R16, N.FORMAT_RG16, N.FORMAT_R16_SNORM, N.FORMAT_RG16_SNORM)
        channel = check_channel(channel, self._texel_layout()[0])
        level = check_level(level, 65535 if norm16 else 255)
        h = C.c_void_p()
        if _scan_words is None:
            N.check(N.lib().vpt_volume_surface(self.texture, channel, level, C.byref(h)))
        else:
            N.check(N.lib().vpt_volume_surface_capped(self.texture, channel, level, int(_scan_words), C.byref(h)))
        return Surface(h)

    # ---- extension: resampling to any grid size (include/vpt.h; DESIGN.md "Resampling") ----
    def resample(self, width, height, depth, mode='filtered'):
        """A new, ready volume in this volume's format and with its filter on a grid of width x height x depth texels (each 1 .. 4096) that
        fills the same cube: 'filtered' (R8, RG8, R16, RG16) interpolates linearly along an axis that grows and averages areas along one
        that shrinks, in integers with one rounding; 'nearest' (every unpacked format) copies the texel under each result texel's centre:
        the mode for labels and masks (vpt_amd.resample_texels states both), derived on the device.  This volume is not changed."""
        from .resample import check_mode, check_size
        code = check_mode(mode)
        width, height, depth = check_size(width, height, depth)
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_resample(self.texture, width, height, depth, code, C.byref(h)))
        return self._same_format(h, {'width': width, 'height': height, 'depth': depth})

    def resample_timed(self, width, height, depth, mode='filtered'):
        """(for measurements) (the volume ``resample`` gives, {'x', 'yz'}: milliseconds of the row pass and of the plane pass of 'filtered',
        the stream drained after each; zeros for 'nearest')"""
        from .resample import check_mode, check_size
        code = check_mode(mode)
        width, height, depth = check_size(width, height, depth)
        h = C.c_void_p()
        ms = (C.c_double * N.RESAMPLE_PHASES)()
        N.check(N.lib().vpt_volume_resample_timed(self.texture, width, height, depth, code, C.byref(h), ms))
        return self._same_format(h, {'width': width, 'height': height, 'depth': depth}), dict(zip(('x', 'yz'), ms))

    def isotropic(self, spacing, pitch=None, mode='filtered'):
        """``resample`` to cubic voxels of edge ``pitch`` (None: the smallest spacing) from this volume's voxel ``spacing`` = (sx, sy, sz):
        the grid vpt_amd.isotropic_shape gives"""
        from .resample import isotropic_shape
        dims = self.modality['dimensions']
        return self.resample(*isotropic_shape((dims['width'], dims['height'], dims['depth']), spacing, pitch), mode=mode)

    # ---- extension: two volumes combined or compared texel by texel (include/vpt.h; DESIGN.md "Combining two volumes") ----
    def _combine_params(self, other, op, channel, params):
        """the CombineParams of ``combine(other, op, channel, **params)``, checked as vpt_amd.combine_texels checks them"""
        from .combine import check_op, check_channel, check_weights, check_mask
        code = check_op(op)
        if not isinstance(other, Volume) or not other.texture or not self.texture:
            raise ValueError('combine takes two ready volumes')
        unknown = set(params) - {'lo', 'hi', 'fill', 'wa', 'wb', 'offset'}
        if unknown:
            raise ValueError('combine takes lo, hi, fill (mask) and wa, wb, offset (blend), not %s' % ', '.join(sorted(unknown)))
        other_channels, other_dtype = other._texel_layout()
        p = N.CombineParams(op=code, b_channel=check_channel(channel, other_channels))
        largest = 65535 if self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16) else 255
        if op == 'mask':
            largest_b = 65535 if np.dtype(other_dtype).itemsize == 2 else 255
            hi = params['hi'] if params.get('hi') is not None else largest_b
            p.lo, p.hi, p.fill = check_mask(params.get('lo', 0), hi, params.get('fill', 0), largest_b, largest)
        elif op == 'blend':
            p.wa, p.wb, p.offset = check_weights(params.get('wa', 256), params.get('wb', 0), params.get('offset', 0))
        return p

    def _combined(self, handle, op):
        out = self._same_format(handle, self.modality['dimensions'])
        if op == 'pair':
            norm16 = self.native_format()[0] == N.FORMAT_R16
            out.modality.update({'format': GL_RG, 'internalFormat': GL_RG16_EXT if norm16 else GL_RG8,
                                 'type': GL_UNSIGNED_SHORT if norm16 else GL_UNSIGNED_BYTE})
        return out

    def combine(self, other, op, channel=0, **params):
        """A new, ready volume on this (R8 / R16) volume's context and with its filter: this volume's texels A combined with the texels B of
        channel ``channel`` of ``other`` (R8, RG8, R16, RG16; same size; may be this volume) by ``op``: 'mask' (lo, hi, fill), 'min', 'max',
        'absdiff', 'blend' (wa, wb, offset) in this volume's format, or 'pair', the RG8 / RG16 volume (A, B) (vpt_amd.combine_texels states
        them), derived on the device.  Neither volume is changed."""
        p = self._combine_params(other, op, channel, params)
        h = C.c_void_p()
        N.check(N.lib().vpt_volume_combine(self.texture, other.texture, C.byref(p), C.byref(h)))
        return self._combined(h, op)

    def combine_timed(self, other, op, channel=0, **params):
        """(for measurements) (the volume ``combine`` gives, the milliseconds of the combining pass alone, the stream drained around it)"""
        p = self._combine_params(other, op, channel, params)
        h = C.c_void_p()
        ms = C.c_double(0)
        N.check(N.lib().vpt_volume_combine_timed(self.texture, other.texture, C.byref(p), C.byref(h), C.byref(ms)))
        return self._combined(h, op), ms.value

    def mask(self, other, lo, hi, fill=0, channel=0):
        """this volume's codes where lo <= B <= hi, ``fill`` elsewhere; ``other`` may be 8- or 16-bit whatever this volume is"""
        return self.combine(other, 'mask', channel, lo=lo, hi=hi, fill=fill)

    def minimum(self, other, channel=0):
        return self.combine(other, 'min', channel)

    def maximum(self, other, channel=0):
        return self.combine(other, 'max', channel)

    def absdiff(self, other, channel=0):
        return self.combine(other, 'absdiff', channel)

    def blend(self, other, wa, wb, offset=0, channel=0):
        """clamp(((wa A + wb B + 128) >> 8) + offset, 0, M): weights in 1/256 units; (256, 256) adds, (256, -256) subtracts, (128, 128)
        averages, (-256, 0, M) inverts, (512, -256) against ``smooth()`` is unsharp masking"""
        return self.combine(other, 'blend', channel, wa=wa, wb=wb, offset=offset)

    def pair(self, other, channel=0):
        """the RG8 / RG16 volume (A, B): ``other`` becomes the second axis of the 2-D transfer function"""
        return self.combine(other, 'pair', channel)

    def compare(self, other, a_range=None, b_range=None, channel=0):
        """{'voxels', 'differing', 'max_abs', 'sum_abs', 'sum_sq', 'in_a', 'in_b', 'both'}: exact integers over this (R8 / R16) volume's
        codes A and the codes B of channel ``channel`` of ``other`` (mixed widths are taken), counted on the device; in_a counts
        a_range[0] <= A <= a_range[1] (None: every code), in_b likewise, both their intersection; plus 'dice', 'jaccard', 'mse', 'psnr' in
        IEEE double, None where a denominator is 0 (vpt_amd.compare_stats states all of it).  More than 2^32 - 1 voxels raise VptError
        (ERR_UNSUPPORTED)."""
        from .combine import check_channel, check_compare_range, ratios, STATS
        if not isinstance(other, Volume) or not other.texture or not self.texture:
            raise ValueError('compare takes two ready volumes')
        other_channels, other_dtype = other._texel_layout()
        channel = check_channel(channel, other_channels)
        largest_a = 65535 if self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16) else 255
        largest_b = 65535 if np.dtype(other_dtype).itemsize == 2 else 255
        lo_a, hi_a = check_compare_range(a_range, largest_a, 'a_range')
        lo_b, hi_b = check_compare_range(b_range, largest_b, 'b_range')
        out = (C.c_uint64 * 8)()
        N.check(N.lib().vpt_volume_compare(self.texture, other.texture, channel, lo_a, hi_a, lo_b, hi_b, out))
        stats = dict(zip(STATS, (int(v) for v in out)))
        stats.update(ratios(stats, max(largest_a, largest_b)))
        return stats

    # ---- extension: morphological reconstruction and the geodesic operations (include/vpt.h; DESIGN.md "Geodesic reconstruction") ----
    def _one_channel(self, handle):
        """the ready one-channel R8 / R16 Volume around a native volume derived from this (R8, RG8, R16 or RG16) one"""
        norm16 = self.native_format()[0] in (N.FORMAT_R16, N.FORMAT_RG16)
        modality = dict(self.modality, format=GL_RED, internalFormat=GL_R16_EXT if norm16 else GL_R8,
                        type=GL_UNSIGNED_SHORT if norm16 else GL_UNSIGNED_BYTE)
        return _derived_volume(type(self)(self._gl), handle, modality, (self.metadata or {}).get('meta', {}), self.modality['dimensions'])

    def _reconstruct(self, mask, op, connectivity, channel, mask_channel, timed, tile_rounds=None):
        from .components import check_connectivity
        from .reconstruct import check_reconstruct_op, check_source_channel
        code, connectivity = check_reconstruct_op(op), check_connectivity(connectivity)
        if not isinstance(mask, Volume) or not mask.texture or not self.texture:
            raise ValueError('reconstruct takes two ready volumes')
        channel = check_source_channel(channel, self._texel_layout()[0])
        mask_channel = check_source_channel(mask_channel, mask._texel_layout()[0])
        h, ms, launches, runs = C.c_void_p(), C.c_double(0), C.c_uint32(0), C.c_uint64(0)
        L = N.lib()
        if tile_rounds is not None:
            N.check(L.vpt_volume_reconstruct_capped(self.texture, channel, mask.texture, mask_channel, code, connectivity, int(tile_rounds), C.byref(h),
                                                    C.byref(ms), C.byref(launches)))
        elif timed:
            N.check(L.vpt_volume_reconstruct_timed(self.texture, channel, mask.texture, mask_channel, code, connectivity, C.byref(h), C.byref(ms),
                                                   C.byref(launches), C.byref(runs)))
        else:
            N.check(L.vpt_volume_reconstruct(self.texture, channel, mask.texture, mask_channel, code, connectivity, C.byref(h)))
            return self._one_channel(h)
        return self._one_channel(h), {'ms': ms.value, 'launches': launches.value, 'tile_runs': runs.value}

    def reconstruct(self, mask, op='dilation', connectivity=6, channel=0, mask_channel=0):
        """A new, ready one-channel R8 / R16 volume on this volume's context and with its filter: the morphological reconstruction, by
        'dilation' or 'erosion', of channel ``channel`` of this volume (the marker) under channel ``mask_channel`` of ``mask`` (R8, RG8, R16,
        RG16 either; same size and channel width; may be this volume) with 6-, 18- or 26-connectivity (vpt_amd.reconstruct_texels states
        it), propagated on the device.  Neither volume is changed."""
        return self._reconstruct(mask, op, connectivity, channel, mask_channel, False)

    def reconstruct_timed(self, mask, op='dilation', connectivity=6, channel=0, mask_channel=0, _tile_rounds=None):
        """(for measurements) (the volume ``reconstruct`` gives, {'ms': the milliseconds of the call up to the result's finalize, the
        stream drained either side, 'launches': the launches of the propagation kernel, 'tile_runs': the tiles that worked, summed over
        them}).  ``_tile_rounds`` (for tests): the rounds a tile may make per launch, through vpt_volume_reconstruct_capped (no tile_runs)."""
        return self._reconstruct(mask, op, connectivity, channel, mask_channel, True, _tile_rounds)

    def _geodesic(self, op, h, connectivity, channel, timed):
        from .components import check_connectivity
        from .reconstruct import check_geodesic_op, check_h, check_source_channel
        code, connectivity = check_geodesic_op(op), check_connectivity(connectivity)
        if not self.texture:
            raise ValueError('a geodesic operation takes a ready volume')
        channels, dtype = self._texel_layout()
        channel = check_source_channel(channel, channels)
        h = check_h(op, h, 65535 if np.dtype(dtype).itemsize == 2 else 255)
        out = C.c_void_p()
        if not timed:
            N.check(N.lib().vpt_volume_geodesic(self.texture, channel, code, h, connectivity, C.byref(out)))
            return self._one_channel(out)
        ms, launches, runs = C.c_double(0), C.c_uint32(0), C.c_uint64(0)
        N.check(N.lib().vpt_volume_geodesic_timed(self.texture, channel, code, h, connectivity, C.byref(out), C.byref(ms), C.byref(launches), C.byref(runs)))
        return self._one_channel(out), {'ms': ms.value, 'launches': launches.value, 'tile_runs': runs.value}

    def geodesic(self, op, h=0, connectivity=6, channel=0):
        """A new, ready one-channel R8 / R16 volume on this (R8, RG8, R16 or RG16) volume's context and with its filter: the geodesic
        operation ``op`` ('fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima'; ``h`` for 'hmax', 'hmin' and 'dome')
        of channel ``channel`` (vpt_amd.geodesic_texels states them), on the device.  This volume is not changed."""
        return self._geodesic(op, h, connectivity, channel, False)

    def geodesic_timed(self, op, h=0, connectivity=6, channel=0):
        """(for measurements) (the volume ``geodesic`` gives, {'ms', 'launches', 'tile_runs'} as ``reconstruct_timed``)"""
        return self._geodesic(op, h, connectivity, channel, True)

    def fill_holes(self, connectivity=6, channel=0):
        """every regional minimum not connected to the volume's border (by ``connectivity``) raised to its rim"""
        return self.geodesic('fill_holes', 0, connectivity, channel)

    def fill_holes_timed(self, connectivity=6, channel=0):
        return self.geodesic_timed('fill_holes', 0, connectivity, channel)

    def clear_border(self, connectivity=6, channel=0):
        """what is connected to the volume's border removed, grey values kept: src - R_d(border marker, src)"""
        return self.geodesic('clear_border', 0, connectivity, channel)

    def clear_border_timed(self, connectivity=6, channel=0):
        return self.geodesic_timed('clear_border', 0, connectivity, channel)

    def hmax(self, h, connectivity=6, channel=0):
        """maxima shallower than ``h`` suppressed: R_d(max(src - h, 0), src)"""
        return self.geodesic('hmax', h, connectivity, channel)

    def hmax_timed(self, h, connectivity=6, channel=0):
        return self.geodesic_timed('hmax', h, connectivity, channel)

    def hmin(self, h, connectivity=6, channel=0):
        """minima shallower than ``h`` suppressed: R_e(min(src + h, M), src)"""
        return self.geodesic('hmin', h, connectivity, channel)

    def hmin_timed(self, h, connectivity=6, channel=0):
        return self.geodesic_timed('hmin', h, connectivity, channel)

    def dome(self, h, connectivity=6, channel=0):
        """src - hmax(h): the caps of height at most ``h`` on the maxima"""
        return self.geodesic('dome', h, connectivity, channel)

    def dome_timed(self, h, connectivity=6, channel=0):
        return self.geodesic_timed('dome', h, connectivity, channel)

    def regional_maxima(self, connectivity=6, channel=0):
        """M on the plateaus without a higher neighbour, 0 elsewhere (a voxel of code 0 is never a maximum)"""
        return self.geodesic('maxima', 0, connectivity, channel)

    def regional_maxima_timed(self, connectivity=6, channel=0):
        return self.geodesic_timed('maxima', 0, connectivity, channel)

    def regional_minima(self, connectivity=6, channel=0):
        """M on the plateaus without a lower neighbour, 0 elsewhere (a voxel of code M is never a minimum)"""
        return self.geodesic('minima', 0, connectivity, channel)

    def regional_minima_timed(self, connectivity=6, channel=0):
        return self.geodesic_timed('minima', 0, connectivity, channel)

    # ---- extension: watershed by steepest descent on a lower-completed relief (include/vpt.h; DESIGN.md "Watershed") ----
    def _watershed(self, lo, hi, polarity, connectivity, min_voxels, channel, texels, timed, caps):
        from .components import check_connectivity, check_min_voxels, check_range
        from .reconstruct import check_source_channel
        from .watershed import check_polarity
        if not self.texture:
            raise ValueError('a watershed takes a ready volume')
        channels, dtype = self._texel_layout()
        norm16 = np.dtype(dtype).itemsize == 2
        channel = check_source_channel(channel, channels)
        lo, hi = check_range(lo, hi, 65535 if norm16 else 255)
        polarity, connectivity, min_voxels = check_polarity(polarity), check_connectivity(connectivity), check_min_voxels(min_voxels)
        if texels is not None and (not isinstance(texels, Volume) or not texels.texture):
            raise ValueError('watershed takes a ready volume as texels')
        args = (self.texture, channel, texels.texture if texels is not None else None, lo, hi, polarity, connectivity, min_voxels)
        h, ms, launches = C.c_void_p(), (C.c_double * N.WATERSHED_PHASES)(), C.c_uint32(0)
        if caps is not None:
            merge_steps, flatten_steps, tile_rounds = caps
            N.check(N.lib().vpt_volume_watershed_capped(*(args + (int(merge_steps), int(flatten_steps), int(tile_rounds), C.byref(h), ms, C.byref(launches)))))
        elif timed:
            N.check(N.lib().vpt_volume_watershed_timed(*(args + (C.byref(h), ms, C.byref(launches)))))
        else:
            N.check(N.lib().vpt_volume_watershed(*(args + (C.byref(h),))))
        # the handle speaks of the volume whose texels it holds: `texels`, or the chosen channel of this one
        basins = Components(texels if texels is not None else (self if channels == 1 else _OneChannelOf(self, norm16)), h)
        if not timed:
            return basins
        return basins, {'ms': dict(zip(('classify', 'plateau', 'links'), ms)), 'plateau_launches': launches.value}

    def watershed(self, lo, hi, polarity='minima', connectivity=6, min_voxels=1, channel=0, texels=None, _caps=None):
        """The basins of channel ``channel`` of this (R8, RG8, R16 or RG16) volume, the relief, over the domain of the codes lo .. hi, as a
        ``Components`` object: the watershed by steepest descent on the lower completion, flooded from the 'minima' or from the 'maxima'
        (a depth channel), on the device (vpt_amd.watershed_texels states the contract).  Every voxel of the domain belongs to exactly one
        basin; ``info``, ``list``, ``ranks``, ``keep``, ``label``, ``measure`` and ``keep_set`` work as on components.  ``texels`` (an R8 /
        R16 volume of this size and channel width; None: the relief's channel) is what ``keep``, ``keep_set`` and ``label`` emit.  Neither
        volume is changed; both may be destroyed.  ``_caps`` (for tests): (merge_steps, flatten_steps, tile_rounds) of
        vpt_volume_watershed_capped."""
        return self._watershed(lo, hi, polarity, connectivity, min_voxels, channel, texels, False, _caps)

    def watershed_timed(self, lo, hi, polarity='minima', connectivity=6, min_voxels=1, channel=0, texels=None, _caps=None):
        """(for measurements) (the basins ``watershed`` gives, {'ms': {'classify', 'plateau', 'links'} in milliseconds, 'plateau_launches'});
        the common tail is the basins' ``profile()``.  ``_caps`` (for tests): (merge_steps, flatten_steps, tile_rounds) of
        vpt_volume_watershed_capped."""
        return self._watershed(lo, hi, polarity, connectivity, min_voxels, channel, texels, True, _caps)

    def _split(self, lo, hi, h, steps, connectivity, min_voxels, timed):
        norm16 = np.dtype(self._texel_layout()[1]).itemsize == 2
        d = self.distance(lo, hi, 'rest')
        try:
            depth = d.channel(steps)
        finally:
            d.destroy()
        try:
            flattened = depth.hmax(h, connectivity, channel=1)
        finally:
            depth.destroy()
        try:
            return flattened._watershed(1, 65535 if norm16 else 255, 'maxima', connectivity, min_voxels, 0, self, timed, None)
        finally:
            flattened.destroy()

    def split(self, lo, hi, h=2, steps=4, connectivity=26, min_voxels=1):
        """The structures of the codes lo .. hi of this (R8 / R16) volume with touching ones split, as a ``Components`` object whose
        emitters speak of this volume: the watershed, from the maxima, of the depth inside the structures (``steps`` rows a voxel) with
        maxima shallower than ``h`` suppressed: distance(lo, hi, 'rest') -> channel(steps) -> hmax(h, connectivity, channel=1) ->
        watershed(1, M, 'maxima', connectivity, min_voxels, texels=self), all on the device (vpt_amd.split_texels states it).  The
        intermediates are destroyed."""
        return self._split(lo, hi, h, steps, connectivity, min_voxels, False)

    def split_timed(self, lo, hi, h=2, steps=4, connectivity=26, min_voxels=1):
        """(for measurements) (the basins ``split`` gives, what ``watershed_timed`` reports of its watershed step)"""
        return self._split(lo, hi, h, steps, connectivity, min_voxels, True)

    def set_wide_tables(self, wide):
        """force the > 4 GiB addressing variant of the kernels (automatic above 4 GiB of bricked data)"""
        N.check(N.lib().vpt_volume_set_wide_tables(self.texture, 1 if wide else 0))

    def bricked_bytes(self):
        n = C.c_uint64(0)
        N.check(N.lib().vpt_volume_bricked_bytes(self.texture, C.byref(n)))
        return n.value


class _OneChannelOf:
    """what ``_VoxelField`` reads of its source, for one channel of a two-channel volume: the description of an R8 / R16 volume"""

    def __init__(self, source, norm16):
        self._gl = source._gl
        self.modality = dict(source.modality, format=GL_RED, internalFormat=GL_R16_EXT if norm16 else GL_R8,
                             type=GL_UNSIGNED_SHORT if norm16 else GL_UNSIGNED_BYTE)
        self.metadata = source.metadata


class _VoxelField:
    """What ``Components`` and ``Distance`` share: the native handle of one uint32 per voxel over a snapshot of an R8 / R16 volume, the box
    read-back of those values and the description of the volumes derived from them.  A subclass names its native functions and the noun of
    the message raised once it has been destroyed."""
    _noun = _destroy = _read = None

    def __init__(self, source, handle):
        self._h = handle
        self._gl = source._gl
        dims = source.modality['dimensions']
        self._shape = (dims['depth'], dims['height'], dims['width'])
        self._norm16 = source.modality.get('internalFormat') == GL_R16_EXT
        # what a derived volume's description is made from (_derived_volume)
        self._modality = dict(source.modality)
        self._meta = dict((source.metadata or {}).get('meta', {}))

    def _handle(self):
        if not self._h:
            raise RuntimeError('the %s have been destroyed' % self._noun)
        return self._h

    def destroy(self):
        if self._h:
            getattr(N.lib(), self._destroy)(self._h)
            self._h = None

    def _values(self, x, y, z, w, h, d):
        """uint32 [d][h][w]: the values of a box of voxels (the whole volume by default)"""
        w = self._shape[2] - x if w is None else w
        h = self._shape[1] - y if h is None else h
        d = self._shape[0] - z if d is None else d
        out = np.empty((int(d), int(h), int(w)), np.uint32)
        N.check(getattr(N.lib(), self._read)(self._handle(), int(x), int(y), int(z), int(w), int(h), int(d), out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def _derived(self, handle, pair=False):
        """the ready Volume around a native volume derived from the field: of the source's format, or (``pair``) RG8 / RG16"""
        out = _derived_volume(Volume(self._gl), handle, self._modality, self._meta, self._modality['dimensions'])
        if pair:
            out.modality.update({'format': GL_RG, 'internalFormat': GL_RG16_EXT if self._norm16 else GL_RG8,
                                 'type': GL_UNSIGNED_SHORT if self._norm16 else GL_UNSIGNED_BYTE})
        return out


class Components(_VoxelField):
    """The connected components of a value range of a volume (``Volume.components``): per-voxel ranks and the component list on the device.
    Label once, select several times.  Outlives the volume it was made from; ``destroy()`` frees the device memory."""
    _noun, _destroy, _read = 'components', 'vpt_components_destroy', 'vpt_components_ranks'

    @property
    def info(self):
        """{'listed', 'dropped', 'foreground_voxels', 'listed_voxels'}"""
        i = N.ComponentsInfo()
        N.check(N.lib().vpt_components_info(self._handle(), C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in N.ComponentsInfo._fields_}

    def list(self, first=0, n=None):
        """[(root_x, root_y, root_z, voxels)] of the components first .. first + n - 1 of the canonical order (n None: to the end)"""
        if n is None:
            n = max(self.info['listed'] - int(first), 0)
        buf = (N.Component * max(int(n), 1))()
        N.check(N.lib().vpt_components_list(self._handle(), int(first), int(n), buf))
        return [(c.root_x, c.root_y, c.root_z, c.voxels) for c in buf[:int(n)]]

    def ranks(self, x=0, y=0, z=0, w=None, h=None, d=None):
        """uint32 [d][h][w]: the ranks of a box of voxels (the whole volume by default)"""
        return self._values(x, y, z, w, h, d)

    def keep(self, first=1, last=None, fill=0):
        """A new, ready volume of the source's size, format and filter: the source's code where first <= rank <= last (last None: every
        rank), ``fill`` elsewhere (vpt_amd.keep_texels states it)"""
        from .components import check_keep
        first, last, fill = check_keep(first, last, fill, 65535 if self._norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_components_keep(self._handle(), first, last, fill, C.byref(h)))
        return self._derived(h)

    def label(self):
        """A new, ready RG8 / RG16 volume with the source's filter: (code, min(rank, M)) (vpt_amd.label_texels states it): the rows of a 2-D
        transfer function select the structures"""
        h = C.c_void_p()
        N.check(N.lib().vpt_components_label(self._handle(), C.byref(h)))
        return self._derived(h, pair=True)

    def _measure_args(self, first, n, values, channel):
        from .measure import check_window, MEASURE_DTYPE
        first, n = check_window(first, n, self.info['listed'])
        if values is not None and (not isinstance(values, Volume) or not values.texture):
            raise ValueError('measure takes a ready volume as values')
        if isinstance(channel, bool) or not isinstance(channel, (int, np.integer)):
            raise ValueError('channel is 0 or 1, not %r' % (channel,))
        out = np.zeros(n, MEASURE_DTYPE)
        return (self._handle(), values.texture if values is not None else None, int(channel), first, n,
                out.ctypes.data_as(C.POINTER(N.ComponentMeasure))), out

    def measure(self, first=0, n=None, values=None, channel=0):
        """A structured array (vpt_amd.MEASURE_DTYPE), one record per component of rank first + 1 .. first + n (n None: to the end of the
        list): voxels, bounding box, index sums, min / max / sum / sum of squares of channel ``channel`` of ``values`` (an R8, RG8, R16 or
        RG16 volume of this size; None: the labelled texels themselves) under the component, and its surface in voxel faces, all exact
        integers counted on the device (vpt_amd.measure_texels states them; vpt_amd.derive gives centroid, mean, variance, extents)."""
        args, out = self._measure_args(first, n, values, channel)
        N.check(N.lib().vpt_components_measure(*args))
        return out

    def measure_timed(self, first=0, n=None, values=None, channel=0):
        """(for measurements) (the records ``measure`` gives, the milliseconds of the measuring pass alone, the stream drained around it)"""
        args, out = self._measure_args(first, n, values, channel)
        ms = C.c_double(0)
        N.check(N.lib().vpt_components_measure_timed(*(args + (C.byref(ms),))))
        return out, ms.value

    def keep_set(self, ranks, fill=0):
        """A new, ready volume of the source's size, format and filter: the source's code where the voxel's rank is in ``ranks`` (an
        iterable of 1-based ranks; duplicates and ranks beyond the list are allowed; or a boolean array with one entry per listed
        component), ``fill`` elsewhere (vpt_amd.keep_set_texels states it)"""
        from .components import check_keep
        from .measure import check_rank_set
        ranks = check_rank_set(ranks, self.info['listed'])
        fill = check_keep(1, None, fill, 65535 if self._norm16 else 255)[2]
        buf = (C.c_uint64 * max(len(ranks), 1))(*ranks)
        h = C.c_void_p()
        N.check(N.lib().vpt_components_keep_set(self._handle(), buf, len(ranks), fill, C.byref(h)))
        return self._derived(h)

    def profile(self):
        """(for measurements) ({phase: milliseconds}, merge launches, flatten launches) of the labelling"""
        ms = (C.c_double * N.COMPONENTS_PHASES)()
        launches = (C.c_uint32 * 2)()
        N.check(N.lib().vpt_components_profile(self._handle(), ms, launches))
        names = ('tiles', 'merge', 'flatten', 'sizes', 'compaction', 'sort', 'ranks')
        return dict(zip(names, ms)), int(launches[0]), int(launches[1])


class Distance(_VoxelField):
    """The squared Euclidean distances to a value range of a volume, or to its complement (``Volume.distance``): one uint32 per voxel on
    the device.  Transform once, select several times.  Outlives the volume it was made from; ``destroy()`` frees the device memory."""
    _noun, _destroy, _read = 'distances', 'vpt_distance_destroy', 'vpt_distance_squared'

    @property
    def info(self):
        """{'seeds', 'largest'}: the number of seeds; the largest finite squared distance, 0 without a seed"""
        i = N.DistanceInfo()
        N.check(N.lib().vpt_distance_info(self._handle(), C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in N.DistanceInfo._fields_}

    def squared(self, x=0, y=0, z=0, w=None, h=None, d=None):
        """uint32 [d][h][w]: the squared distances of a box of voxels (the whole volume by default); 0xFFFFFFFF: there is no seed"""
        return self._values(x, y, z, w, h, d)

    def within(self, r2_lo=0, r2_hi=None, fill=0):
        """A new, ready volume of the source's size, format and filter: the source's code where r2_lo <= d2 <= r2_hi (r2_hi None:
        0xFFFFFFFF), ``fill`` elsewhere (vpt_amd.within_texels states it)"""
        from .distance import check_within
        r2_lo, r2_hi, fill = check_within(r2_lo, r2_hi, fill, 65535 if self._norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_distance_within(self._handle(), r2_lo, r2_hi, fill, C.byref(h)))
        return self._derived(h)

    def channel(self, steps=1):
        """A new, ready RG8 / RG16 volume with the source's filter: (code, min(isqrt(steps^2 d2), M)) (vpt_amd.channel_texels states it):
        the second axis of a 2-D transfer function is the distance, ``steps`` rows a voxel"""
        from .distance import check_steps
        h = C.c_void_p()
        N.check(N.lib().vpt_distance_channel(self._handle(), check_steps(steps), C.byref(h)))
        return self._derived(h, pair=True)

    def _sibling(self, handle):
        """a ``Distance`` around another native handle over the same snapshot"""
        other = Distance.__new__(Distance)
        other.__dict__.update(self.__dict__)
        other._modality, other._meta = dict(self._modality), dict(self._meta)
        other._h = handle
        return other

    def thickness(self):
        """The local thickness, as another ``Distance`` object whose values are T2: per voxel the largest squared distance D(c) among the
        open balls { |v - c|^2 < D(c) } of these distances that hold the voxel, 0 where none does (vpt_amd.thickness_squared_texels states
        it), on the device.  ``within(r^2 + 1, None)`` of the result is the opening by the Euclidean ball of radius r, ``channel(2)`` the
        local diameter.  This object is not changed and may be destroyed."""
        h = C.c_void_p()
        N.check(N.lib().vpt_distance_thickness(self._handle(), C.byref(h)))
        return self._sibling(h)

    def thickness_timed(self, _flags=None):
        """(for measurements) (what ``thickness`` gives, {'ms': {'tiles', 'cover', 'info'} in milliseconds, 'tiles': the tiles that hold a
        centre, 'visited': the centre tiles their workgroups ran over}).  ``_flags`` (for tests): the flags of
        vpt_distance_thickness_capped (1: no value cull, 2: no reach cull); 'tiles' is then None."""
        h = C.c_void_p()
        ms = (C.c_double * N.THICKNESS_PHASES)()
        tiles, visited = C.c_uint64(0), C.c_uint64(0)
        if _flags is None:
            N.check(N.lib().vpt_distance_thickness_timed(self._handle(), C.byref(h), ms, C.byref(tiles), C.byref(visited)))
        else:
            N.check(N.lib().vpt_distance_thickness_capped(self._handle(), int(_flags), C.byref(h), ms, C.byref(visited)))
        return self._sibling(h), {'ms': dict(zip(('tiles', 'cover', 'info'), ms)), 'tiles': None if _flags is not None else int(tiles.value),
                                  'visited': int(visited.value)}

    def profile(self):
        """(for measurements) {'x', 'y', 'z'}: milliseconds of the three passes of the transform"""
        ms = (C.c_double * N.DISTANCE_PHASES)()
        N.check(N.lib().vpt_distance_profile(self._handle(), ms))
        return dict(zip(('x', 'y', 'z'), ms))


class Skeleton(_VoxelField):
    """The burn passes of a thinning of a value range of a volume (``Volume.skeleton``): one uint32 per voxel on the device, 0 outside the
    range, k for a voxel deleted in pass k, KEPT for a voxel that survived.  Thin once, select several times.  Outlives the volume it was
    made from; ``destroy()`` (or ``close()``) frees the device memory."""
    _noun, _destroy, _read = 'burn passes', 'vpt_skeleton_destroy', 'vpt_skeleton_burn'
    KEPT = N.THIN_KEPT

    @property
    def info(self):
        """{'object_voxels', 'kept_voxels', 'passes', 'converged', 'isolated', 'ends', 'regular', 'junctions'}: the last four count the kept
        voxels with 0, 1, 2 and >= 3 kept 26-neighbours"""
        i = N.SkeletonInfo()
        N.check(N.lib().vpt_skeleton_info(self._handle(), C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in N.SkeletonInfo._fields_}

    def burn(self, x=0, y=0, z=0, w=None, h=None, d=None):
        """uint32 [d][h][w]: the burn passes of a box of voxels (the whole volume by default)"""
        return self._values(x, y, z, w, h, d)

    def within(self, k_lo=N.THIN_KEPT, k_hi=None, fill=0):
        """A new, ready volume of the source's size, format and filter: the source's code where k_lo <= burn pass <= k_hi (k_hi None:
        0xFFFFFFFF), ``fill`` elsewhere (vpt_amd.burn_within_texels states it).  ``within(k)`` is the object after k - 1 passes."""
        from .skeleton import check_within
        k_lo, k_hi, fill = check_within(k_lo, k_hi, fill, 65535 if self._norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_skeleton_within(self._handle(), k_lo, k_hi, fill, C.byref(h)))
        return self._derived(h)

    def volume(self):
        """The skeleton as a volume: ``within(KEPT, KEPT, 0)``"""
        return self.within(N.THIN_KEPT, N.THIN_KEPT, 0)

    def profile(self):
        """(for measurements) ({'seed', 'border', 'steps', 'census'} in milliseconds, kernel launches, the tiles the sub-step launches
        worked on, summed)"""
        ms = (C.c_double * N.SKELETON_PHASES)()
        launches, tiles = C.c_uint64(0), C.c_uint64(0)
        N.check(N.lib().vpt_skeleton_profile(self._handle(), ms, C.byref(launches), C.byref(tiles)))
        return dict(zip(('seed', 'border', 'steps', 'census'), ms)), int(launches.value), int(tiles.value)

    def graph(self):
        """The graph of the kept voxels as a ``Graph`` object, built on the device (vpt_amd.graph.skeleton_graph_texels states it); its
        emitters and its ``branches`` / ``nodes`` speak in the codes of this skeleton's source.  This object is not changed and may be
        destroyed."""
        h = C.c_void_p()
        N.check(N.lib().vpt_skeleton_graph(self._handle(), C.byref(h)))
        return Graph(_FieldSource(self), h)

    close = _VoxelField.destroy


class _FieldSource:
    """what ``_VoxelField`` reads of its source, for a field made of another field: the description of that field's source"""

    def __init__(self, field):
        self._gl = field._gl
        self.modality = dict(field._modality)
        self.metadata = {'meta': dict(field._meta)}


class Graph(_VoxelField):
    """The graph of a set of voxels (``Volume.graph``, ``Skeleton.graph``): the class of every voxel, the branches and the nodes as two
    labellings and one record per branch and node, on the device.  Build once; list, measure, prune and colour several times.  Outlives
    what it was made from; ``destroy()`` (or ``close()``) frees the device memory (``branches`` and ``nodes`` once taken are the caller's)."""
    _noun, _destroy = 'graph', 'vpt_graph_destroy'

    def __init__(self, source, handle):
        super().__init__(source, handle)
        self._source = _FieldSource(self)
        self._branches = self._nodes = None

    @property
    def info(self):
        """{'kept_voxels', 'node_voxels', 'branches', 'nodes', 'isolated', 'segments', 'spurs', 'links', 'loops', 'cycles', 'steps_face',
        'steps_edge', 'steps_corner', 'attachments'}"""
        i = N.GraphInfo()
        N.check(N.lib().vpt_graph_info(self._handle(), C.byref(i)))
        return {name: int(getattr(i, name)) for name, _ in N.GraphInfo._fields_}

    def _components(self, call):
        h = C.c_void_p()
        N.check(getattr(N.lib(), call)(self._handle(), C.byref(h)))
        return Components(self._source, h)

    @property
    def branches(self):
        """the branches as a ``Components`` object (made at the first use; the caller destroys it): ranks are branch ranks, texels the
        source's codes, so ``measure``, ``keep_set``, ``keep`` and ``label`` work on branches unchanged"""
        if self._branches is None:
            self._branches = self._components('vpt_graph_branch_components')
        return self._branches

    @property
    def nodes(self):
        """the nodes as a ``Components`` object (made at the first use; the caller destroys it)"""
        if self._nodes is None:
            self._nodes = self._components('vpt_graph_node_components')
        return self._nodes

    def _records(self, call, count, dtype, ctype, first, n):
        from .measure import check_window
        first, n = check_window(first, n, count)
        out = np.zeros(n, dtype)
        N.check(getattr(N.lib(), call)(self._handle(), first, n, out.ctypes.data_as(C.POINTER(ctype))))
        return out

    def branch_records(self, first=0, n=None):
        """A structured array (vpt_amd.graph.BRANCH_DTYPE), one record per branch of rank first + 1 .. first + n (n None: to the end)"""
        from .graph import BRANCH_DTYPE
        return self._records('vpt_graph_branches', self.info['branches'], BRANCH_DTYPE, N.GraphBranch, first, n)

    def node_records(self, first=0, n=None):
        """A structured array (vpt_amd.graph.NODE_DTYPE), one record per node of rank first + 1 .. first + n (n None: to the end)"""
        from .graph import NODE_DTYPE
        return self._records('vpt_graph_nodes', self.info['nodes'], NODE_DTYPE, N.GraphNode, first, n)

    def lengths(self, spacing=1.0):
        """float64 per branch: (steps_face + sqrt 2 steps_edge + sqrt 3 steps_corner) * spacing; assumes cubic voxels (``Volume.isotropic``)"""
        from .graph import lengths
        return lengths(self.branch_records(), spacing)

    def classes(self):
        """A new, ready RG8 / RG16 volume with the source's filter: (code, class) (vpt_amd.graph.classes_texels states it): a row of a 2-D
        transfer function colours ends (2) and junctions (4)"""
        h = C.c_void_p()
        N.check(N.lib().vpt_graph_classes(self._handle(), C.byref(h)))
        return self._derived(h, pair=True)

    def prune(self, length, weights=(10, 14, 17), debris=False, fill=0):
        """A new, ready volume of the source's size, format and filter: the source's code where the voxel is in the set and its branch is
        not dropped, ``fill`` elsewhere (vpt_amd.graph.prune_texels states it).  A branch is dropped when weights . (steps_face, steps_edge,
        steps_corner) <= length and it is a spur, or (``debris``) a segment or an isolated voxel.  One round, not thinned again; all spurs
        of a node go together."""
        from .graph import check_prune, PRUNE_DEBRIS
        length, (wf, we, wc), flags, fill = check_prune(length, weights, PRUNE_DEBRIS if debris else 0, fill, 65535 if self._norm16 else 255)
        h = C.c_void_p()
        N.check(N.lib().vpt_graph_prune(self._handle(), length, wf, we, wc, flags, fill, C.byref(h)))
        return self._derived(h)

    def profile(self):
        """(for measurements) ({'seed', 'classify', 'branches', 'nodes', 'links', 'host'} in milliseconds, kernel launches of the unit)"""
        ms = (C.c_double * N.GRAPH_PHASES)()
        launches = C.c_uint64(0)
        N.check(N.lib().vpt_graph_profile(self._handle(), ms, C.byref(launches)))
        return dict(zip(('seed', 'classify', 'branches', 'nodes', 'links', 'host'), ms)), int(launches.value)

    close = _VoxelField.destroy


class _DeviceArray:
    """a buffer on the device as torch takes it (the CUDA array interface)"""

    def __init__(self, pointer, shape, owner):
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': '<i4', 'data': (int(pointer), False), 'version': 2, 'strides': None}
        self._owner = owner


class Surface:
    """The surface of a volume at a level as a mesh (``Volume.surface``): uint32 [V][3] vertices in fixed point of 1 / 65536 voxel and
    uint32 [Q][4] quads on the device, in the contract's order.  Extract once, read, measure and write several times.  Outlives the volume
    it was made from; ``destroy()`` (or ``close()``) frees the device memory."""

    def __init__(self, handle):
        self._h = handle

    def _handle(self):
        if not self._h:
            raise RuntimeError('the surface has been destroyed')
        return self._h

    def destroy(self):
        if self._h:
            N.lib().vpt_surface_destroy(self._h)
            self._h = None

    close = destroy

    @property
    def info(self):
        """{'vertices', 'quads', 'cells', 'inside', 'crossings': [x, y, z], 'level', 'width', 'height', 'depth', 'channel'}"""
        i = N.SurfaceInfo()
        N.check(N.lib().vpt_surface_info(self._handle(), C.byref(i)))
        out = {name: int(getattr(i, name)) for name, _ in N.SurfaceInfo._fields_ if name != 'crossings'}
        out['crossings'] = [int(c) for c in i.crossings]
        return out

    def _page(self, read, count, per, first, n):
        from .surface import check_window
        first, n = check_window(first, n, count, 'vertices' if per == 3 else 'quads')
        out = np.empty((n, per), np.uint32)
        N.check(read(self._handle(), first, n, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def vertices(self, first=0, n=None):
        """uint32 [n][3]: the stored coordinates q (x, y, z) of the vertices first .. first + n - 1 (n None: to the end)"""
        return self._page(N.lib().vpt_surface_vertices, self.info['vertices'], 3, first, n)

    def quads(self, first=0, n=None):
        """uint32 [n][4]: the vertex numbers of the quads first .. first + n - 1 (n None: to the end)"""
        return self._page(N.lib().vpt_surface_quads, self.info['quads'], 4, first, n)

    def triangles(self):
        """uint32 [2 Q][3]: (q0, q1, q2) and (q0, q2, q3) of every quad"""
        from .surface import triangles
        return triangles(self.quads())

    def positions(self, spacing=(1, 1, 1), origin=(0, 0, 0)):
        """float64 [V][3]: (q / 65536 - 1) * spacing + origin"""
        from .surface import positions
        return positions(self.vertices(), spacing, origin)

    def area(self, spacing=(1, 1, 1)):
        """float64: the area of the triangles"""
        from .surface import area
        return area(self.vertices(), self.quads(), spacing)

    def volume(self, spacing=(1, 1, 1)):
        """float64: the volume the triangles enclose"""
        from .surface import volume
        return volume(self.vertices(), self.quads(), spacing)

    def normals(self, spacing=(1, 1, 1)):
        """float64 [V][3]: area-weighted, per vertex, pointing from the object to the background"""
        from .surface import normals
        return normals(self.vertices(), self.quads(), spacing)

    def write_stl(self, path, spacing=(1, 1, 1), origin=(0, 0, 0)):
        from .surface import write_stl
        write_stl(path, self.vertices(), self.quads(), spacing, origin)

    def write_ply(self, path, spacing=(1, 1, 1), origin=(0, 0, 0)):
        from .surface import write_ply
        write_ply(path, self.vertices(), self.quads(), spacing, origin)

    def write_obj(self, path, spacing=(1, 1, 1), origin=(0, 0, 0)):
        from .surface import write_obj
        write_obj(path, self.vertices(), self.quads(), spacing, origin)

    def device(self):
        """(vertices, quads): the addresses of the handle's buffers on the device (None for an empty surface), valid until destroy"""
        v, q = C.c_void_p(), C.c_void_p()
        N.check(N.lib().vpt_surface_device(self._handle(), C.byref(v), C.byref(q)))
        return v.value, q.value

    def device_tensors(self):
        """(vertices [V][3], quads [Q][4]) as torch int32 tensors over the handle's own buffers (the uint32 words bit for bit; no
        copy): valid until destroy, to be used on the context's stream or behind a synchronisation of it"""
        import torch
        i = self.info
        v, q = self.device()
        device = torch.device('cuda', torch.cuda.current_device())
        if not i['vertices']:
            return torch.empty((0, 3), dtype=torch.int32, device=device), torch.empty((0, 4), dtype=torch.int32, device=device)
        return (torch.as_tensor(_DeviceArray(v, (i['vertices'], 3), self), device=device),
                torch.as_tensor(_DeviceArray(q, (i['quads'], 4), self), device=device))

    @property
    def profile(self):
        """(for measurements) {'inside', 'classify', 'scan', 'vertices', 'quads'}: milliseconds of the five phases"""
        ms = (C.c_double * N.SURFACE_PHASES)()
        N.check(N.lib().vpt_surface_profile(self._handle(), ms))
        return dict(zip(('inside', 'classify', 'scan', 'vertices', 'quads'), ms))
