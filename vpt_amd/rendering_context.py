"""RenderingContext — src/js/RenderingContext.js:20-229, headless: the caller of the renderer path (SURVEY §8b
"Caller to reproduce").  Same members and methods minus the browser parts (canvas, WebGL context loss, animators,
recording): where the reference blits the tone mapper's texture to the canvas (:199-209), ``getFrame()`` reads it back.
"""
import numpy as np

from .animators import OrbitCameraAnimator
from .context import Context
from .property_bag import EventTarget, CustomEvent
from .renderers import RendererFactory
from .scene import Node, Transform, PerspectiveCamera
from .tonemappers import ToneMapperFactory
from .volume import Volume
from .skeleton import check_skeleton
from .watershed import check_split


class RenderingContext(EventTarget):

    def __init__(self, options=None):
        super().__init__()
        options = options or {}
        # (extension) 'central' | 'sobel': a one-channel R8 / R16 volume gets its gradient magnitude as second channel when it is loaded
        self.gradient = options.get('gradient')
        self.gradientGain = options['gradientGain'] if options.get('gradientGain') is not None else 1.0
        if self.gradient is not None:
            from .gradient import operator_code, gain_factor
            operator_code(self.gradient); gain_factor(self.gradientGain)              # a bad option fails here, not at the first volume
        # (extension) None | [lo, hi] | 'range' | {'percentiles': [a, b]}: a one-channel volume is windowed to R8 ('r8') / R16 ('r16') when it
        # is loaded, before the gradient is derived
        self.window = options.get('window')
        self.windowFormat = options['windowFormat'] if options.get('windowFormat') is not None else 'r8'
        if self.window is not None:
            from .window import format_bits
            format_bits(self.windowFormat); self._window_spec(self.window)             # a bad option fails here, not at the first volume
        # (extension) None | passes 1 .. 8: an R8 / R16 volume is smoothed (binomial 3 x 3 x 3) when it is loaded, behind the window;
        # None | 0 | levels >= 1: the volume is reduced to ceil(n / 2) texels per axis that many times, behind the smoothing and before the gradient
        self.smooth = options.get('smooth')
        self.reduce = options.get('reduce')
        if self.smooth is not None:
            from .pyramid import check_passes
            check_passes(self.smooth)                                                  # a bad option fails here, not at the first volume
        if self.reduce is not None and not (self.reduce == 0 and not isinstance(self.reduce, bool)):
            from .pyramid import check_levels
            check_levels(self.reduce)
        # (extension) None | 'median' | 'erode' | 'dilate' | 'open' | 'close', rankPasses 1 .. 8: an R8 / R16 volume gets that rank filter over
        # the 3 x 3 x 3 box when it is loaded, behind the window and in front of the smoothing
        self.rank = options.get('rank')
        self.rankPasses = options['rankPasses'] if options.get('rankPasses') is not None else 1
        from .rank import operator_code as rank_operator_code, check_passes as check_rank_passes
        if self.rank is not None:
            rank_operator_code(self.rank)                                              # a bad option fails here, not at the first volume
        check_rank_passes(self.rankPasses)
        # (extension) None | {'lo', 'hi', 'connectivity': 6, 'minVoxels': 1, 'mode': 'keep', 'keep': n | None} | {..., 'mode': 'label'}: the
        # connected components of the codes lo .. hi of an R8 / R16 volume.  'keep' runs behind the rank filter and in front of the smoothing:
        # the n largest components (None: all of at least minVoxels voxels) keep their codes, everything else becomes 0.  'label' runs where
        # the gradient runs, on the final scalar volume: the second channel is min(rank, M), so it cannot be combined with `gradient`
        self.components = self._components_spec(options.get('components'))
        if self.components is not None and self.components['mode'] == 'label' and self.gradient is not None:
            raise ValueError("components mode 'label' and gradient both write the second channel: name one of them")
        # (extension) None | {'lo', 'hi', 'seeds': 'range', 'mode': 'within', 'from': 0, 'to': None, 'fill': 0} | {..., 'mode': 'channel',
        # 'steps': 1}: the exact squared Euclidean distance d2 of every voxel of an R8 / R16 volume to the codes lo .. hi (seeds 'range') or
        # to the codes outside them (seeds 'rest').  'within' runs behind `components` mode 'keep' and in front of the smoothing: the codes
        # with from <= d2 <= to (squared voxels; to None: no upper end) stay, everything else becomes `fill`.  'channel' runs where the
        # gradient runs, on the final scalar volume: the second channel is min(isqrt(steps^2 d2), M), so it cannot be combined with
        # `gradient` or with `components` mode 'label'
        self.distance = self._distance_spec(options.get('distance'))
        if self.distance is not None and self.distance['mode'] == 'channel':
            if self.gradient is not None:
                raise ValueError("distance mode 'channel' and gradient both write the second channel: name one of them")
            if self.components is not None and self.components['mode'] == 'label':
                raise ValueError("distance mode 'channel' and components mode 'label' both write the second channel: name one of them")
        # (extension) None | the keys of `distance`, with seeds 'rest' and steps 2 by default: the local thickness T2 of the structure of the
        # codes lo .. hi (seeds 'rest'; 'range': of its complement), the squared radius of the largest inscribed ball that holds the voxel
        # (Distance.thickness), in the place of d2: 'within' keeps the codes with from <= T2 <= to (from r^2 + 1: the opening by the ball of
        # radius r), 'channel' writes min(isqrt(steps^2 T2), M) (steps 2: the diameter in voxels).  It is applied where `distance` is and
        # conflicts as `distance` does; naming both is refused
        self.thickness = self._distance_spec(options.get('thickness'), 'thickness')
        if self.thickness is not None:
            if self.distance is not None:
                raise ValueError("distance and thickness are two readings of one transform: name one of them")
            if self.thickness['mode'] == 'channel':
                if self.gradient is not None:
                    raise ValueError("thickness mode 'channel' and gradient both write the second channel: name one of them")
                if self.components is not None and self.components['mode'] == 'label':
                    raise ValueError("thickness mode 'channel' and components mode 'label' both write the second channel: name one of them")
        # (extension) None | {'lo', 'hi', 'mode': 'ends', 'passes': 0, 'fill': 0}: the volume is replaced by the skeleton of the codes
        # lo .. hi of an R8 / R16 volume (Volume.skeleton; mode 'kernel' | 'ends' | 'isthmus'): the voxels that survive the thinning keep
        # their codes, everything else becomes `fill`.  It is applied where `thickness` mode 'within' is; naming it together with
        # `distance` or `thickness` mode 'within' is refused
        self.skeleton = check_skeleton(options.get('skeleton'))
        if self.skeleton is not None:
            if self.distance is not None and self.distance['mode'] == 'within':
                raise ValueError("skeleton and distance mode 'within' both replace the volume by a selection of it: name one of them")
            if self.thickness is not None and self.thickness['mode'] == 'within':
                raise ValueError("skeleton and thickness mode 'within' both replace the volume by a selection of it: name one of them")
        # (extension) None | {'size': [w, h, d]} | {'spacing': [sx, sy, sz], 'pitch': None}, plus 'mode': 'filtered' | 'nearest': the volume is
        # resampled to that grid, or to cubic voxels of edge `pitch` (None: the smallest spacing), when it is loaded, behind the window and in
        # front of the rank filter: rank, components and distance see the resampled grid.  A volume whose format the mode does not take is
        # left as it is
        self.resample = self._resample_spec(options.get('resample'))
        # (extension) None | {'reader' | 'volume', 'op', 'channel': 0, 'lo', 'hi', 'fill', 'wa', 'wb', 'offset', 'resample': None | 'nearest' |
        # 'filtered'}: an R8 / R16 volume is combined with a second one when it is loaded (Volume.combine).  A 'reader' is loaded into a second
        # volume and destroyed afterwards, a 'volume' stays the caller's; with 'resample' set and differing sizes the second volume is first
        # resampled to the primary's current grid in that mode.  The one-channel ops run behind `resample` and in front of `rank`; 'pair'
        # runs where the gradient runs, on the final scalar volume, so it cannot be combined with `gradient`, `components` mode 'label' or
        # `distance` mode 'channel'
        self.combine = self._combine_spec(options.get('combine'))
        if self.combine is not None and self.combine['op'] == 'pair':
            if self.gradient is not None:
                raise ValueError("combine op 'pair' and gradient both write the second channel: name one of them")
            if self.components is not None and self.components['mode'] == 'label':
                raise ValueError("combine op 'pair' and components mode 'label' both write the second channel: name one of them")
            if self.distance is not None and self.distance['mode'] == 'channel':
                raise ValueError("combine op 'pair' and distance mode 'channel' both write the second channel: name one of them")
            if self.thickness is not None and self.thickness['mode'] == 'channel':
                raise ValueError("combine op 'pair' and thickness mode 'channel' both write the second channel: name one of them")
        # (extension) None | {'op': 'fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima', 'h': 0, 'connectivity': 6}: an
        # R8 / R16 volume gets that geodesic operation (Volume.geodesic) when it is loaded, behind the rank filter and in front of
        # `components` mode 'keep' and the smoothing
        self.geodesic = self._geodesic_spec(options.get('geodesic'))
        # (extension) None | {'lo', 'hi', 'h': 2, 'steps': 4, 'connectivity': 26, 'minVoxels': 1}: the structures of the codes lo .. hi of an
        # R8 / R16 volume with touching ones split by the watershed of their depth (Volume.split).  It runs where the gradient runs, on the
        # final scalar volume: the second channel is min(rank of the basin, M), so it cannot be combined with `gradient`, `components` mode
        # 'label', `distance` mode 'channel' or `combine` op 'pair'
        self.split = check_split(options.get('split'))
        if self.split is not None:
            if self.gradient is not None:
                raise ValueError("split and gradient both write the second channel: name one of them")
            if self.components is not None and self.components['mode'] == 'label':
                raise ValueError("split and components mode 'label' both write the second channel: name one of them")
            if self.distance is not None and self.distance['mode'] == 'channel':
                raise ValueError("split and distance mode 'channel' both write the second channel: name one of them")
            if self.thickness is not None and self.thickness['mode'] == 'channel':
                raise ValueError("split and thickness mode 'channel' both write the second channel: name one of them")
            if self.combine is not None and self.combine['op'] == 'pair':
                raise ValueError("split and combine op 'pair' both write the second channel: name one of them")
        self.gl = Context(options.get('device', 0))                                   # initGL(), :61-105
        self.environmentTexture = np.array([[[255, 255, 255, 255]]], dtype=np.uint8)   # :90-101
        self._rng = options.get('rng')
        self._resolution = options['resolution'] if options.get('resolution') is not None else 512   # :35
        self.filter = options['filter'] if options.get('filter') is not None else 'linear'           # :36 ('linear' | 'nearest' | 'quasicubic')
        self.camera = Node()                                                          # :38-40
        self.camera.transform.localTranslation = [0, 0, 2]
        self.camera.components.append(PerspectiveCamera(self.camera))
        self.camera.transform.addEventListener('change', lambda e: self.renderer.reset() if self.renderer else None)   # :42-46
        self.volume = Volume(self.gl)                                                 # :56
        self.volumeTransform = Transform(Node())                                      # :57
        self.renderer = None
        self.toneMapper = None
        self.cameraAnimator = OrbitCameraAnimator(self.camera, None)                  # :54 (headless: no canvas to listen on)
        self.resize(*self._size())

    def _size(self):
        r = self._resolution
        return (int(r), int(r)) if isinstance(r, (int, float)) else (int(r[0]), int(r[1]))

    def destroy(self):
        if self.toneMapper:
            self.toneMapper.destroy(); self.toneMapper = None
        if self.renderer:
            self.renderer.destroy(); self.renderer = None
        if self.volume:
            self.volume.destroy()
        self.gl.destroy()

    def resize(self, width, height):                                                  # :117-121
        self.camera.getComponent(PerspectiveCamera).aspect = width / height

    def setVolume(self, reader):                                                      # :123-133
        old = self.volume
        self.volume = Volume(self.gl, reader)
        self.volume.addEventListener('progress', lambda e: self.dispatchEvent(CustomEvent('progress', {'detail': e.detail})))
        self.volume.load()
        self.volume.setFilter(self.filter)
        try:
            if self.window is not None:
                source = self.volume
                lo, hi = self._window_of(source)
                self.volume = source.window(lo, hi, self.windowFormat)                # the transfer function's x axis is [lo, hi]
                source.destroy()
            if self.resample is not None and self._resample_takes(self.volume, self.resample['mode']):
                source = self.volume
                if self.resample['size'] is not None:
                    self.volume = source.resample(*self.resample['size'], mode=self.resample['mode'])
                else:
                    self.volume = source.isotropic(self.resample['spacing'], self.resample['pitch'], self.resample['mode'])
                source.destroy()
            if self.combine is not None and self.combine['op'] != 'pair' and self._one_channel_unorm(self.volume):
                self._combine_with(self.combine)
            if self.rank is not None and self._one_channel_unorm(self.volume):
                source = self.volume
                self.volume = source.rank(self.rank, self.rankPasses)
                source.destroy()
            if self.geodesic is not None and self._one_channel_unorm(self.volume):
                source = self.volume
                self.volume = source.geodesic(self.geodesic['op'], min(self.geodesic['h'], self._largest_code(source)), self.geodesic['connectivity'])
                source.destroy()
            if self.components is not None and self.components['mode'] == 'keep' and self._one_channel_unorm(self.volume):
                self._derive(lambda source, found: found.keep(1, self.components['keep']))
            if self.distance is not None and self.distance['mode'] == 'within' and self._one_channel_unorm(self.volume):
                spec = self.distance
                self._derive_distance(lambda found: found.within(spec['from'], spec['to'], spec['fill']))
            if self.thickness is not None and self.thickness['mode'] == 'within' and self._one_channel_unorm(self.volume):
                spec = self.thickness
                self._derive_distance(lambda found: found.within(spec['from'], spec['to'], spec['fill']), thickness=True)
            if self.skeleton is not None and self._one_channel_unorm(self.volume):
                spec, source = self.skeleton, self.volume
                found = source.skeleton(spec['lo'], min(spec['hi'], self._largest_code(source)), spec['mode'], spec['passes'])
                try:
                    self.volume = found.within(found.KEPT, found.KEPT, min(spec['fill'], self._largest_code(source)))
                finally:
                    found.destroy()
                source.destroy()
            if self.smooth is not None and self._one_channel_unorm(self.volume):
                source = self.volume
                self.volume = source.smooth(self.smooth)
                source.destroy()
            if self.reduce:
                source = self.volume
                self.volume = source.reduce(self.reduce)
                source.destroy()
            if self.gradient is not None and self._one_channel_unorm(self.volume):
                source = self.volume
                self.volume = source.derive_gradient(self.gradient, self.gradientGain)    # (value, gradient magnitude): the 2-D transfer function's axes
                source.destroy()
            if self.components is not None and self.components['mode'] == 'label' and self._one_channel_unorm(self.volume):
                self._derive(lambda source, found: found.label())                     # (value, rank): a row of the 2-D transfer function per structure
            if self.distance is not None and self.distance['mode'] == 'channel' and self._one_channel_unorm(self.volume):
                self._derive_distance(lambda found: found.channel(self.distance['steps']))   # (value, distance): the 2-D transfer function's axes
            if self.thickness is not None and self.thickness['mode'] == 'channel' and self._one_channel_unorm(self.volume):
                self._derive_distance(lambda found: found.channel(self.thickness['steps']), thickness=True)   # (value, local thickness)
            if self.combine is not None and self.combine['op'] == 'pair' and self._one_channel_unorm(self.volume):
                self._combine_with(self.combine)                                      # (value, the second volume): the 2-D transfer function's axes
            if self.split is not None and self._one_channel_unorm(self.volume):
                spec, source = self.split, self.volume
                largest = self._largest_code(source)                                  # the range is open above, and h is at most M
                found = source.split(spec['lo'], min(spec['hi'], largest), min(spec['h'], largest), spec['steps'], spec['connectivity'],
                                     spec['minVoxels'])
                try:
                    self.volume = found.label()                                       # (value, basin): a row of the 2-D transfer function per structure
                finally:
                    found.destroy()
                source.destroy()
        except Exception:                                                             # the context keeps the volume it had
            self.volume.destroy()
            self.volume = old
            raise
        if self.renderer:
            self.renderer.setVolume(self.volume)
        if old:
            old.destroy()                                                             # device memory is not garbage-collected

    def _derive(self, emit):
        """replaces self.volume by what ``emit(source, components of the `components` option)`` returns"""
        spec = self.components
        source = self.volume
        from . import _native as N
        largest = 65535 if source.native_format()[0] == N.FORMAT_R16 else 255        # the range is open above: hi may exceed an R8 volume's codes
        found = source.components(spec['lo'], min(spec['hi'], largest), spec['connectivity'], spec['minVoxels'])
        try:
            self.volume = emit(source, found)
        finally:
            found.destroy()
        source.destroy()

    def _derive_distance(self, emit, thickness=False):
        """replaces self.volume by what ``emit(distances of the `distance` option)`` returns, or (``thickness``)
        ``emit(local thickness of the `thickness` option)``"""
        spec = self.thickness if thickness else self.distance
        source = self.volume
        from . import _native as N
        largest = 65535 if source.native_format()[0] == N.FORMAT_R16 else 255        # the range is open above: hi may exceed an R8 volume's codes
        found = source.distance(spec['lo'], min(spec['hi'], largest), spec['seeds'])
        if thickness:
            depth = found
            try:
                found = depth.thickness()
            finally:
                depth.destroy()
        try:
            self.volume = emit(found)
        finally:
            found.destroy()
        source.destroy()

    def _combine_with(self, spec):
        """replaces self.volume by its combination with the second volume of the `combine` option"""
        source = self.volume
        second, owned = spec['volume'], False
        if second is None:
            second, owned = Volume(self.gl, spec['reader']), True
            second.load()
        try:
            dims, other = source.modality['dimensions'], second.modality['dimensions']
            if spec['resample'] is not None and any(dims[k] != other[k] for k in ('width', 'height', 'depth')):
                fitted = second.resample(dims['width'], dims['height'], dims['depth'], spec['resample'])
                if owned:
                    second.destroy()
                second, owned = fitted, True
            self.volume = source.combine(second, spec['op'], spec['channel'], **spec['params'])
        finally:
            if owned:
                second.destroy()
        source.destroy()

    @staticmethod
    def _largest_code(volume):
        from . import _native as N
        return 65535 if volume.native_format()[0] == N.FORMAT_R16 else 255

    @staticmethod
    def _geodesic_spec(spec):
        """the `geodesic` option with its defaults filled in, or None; raises ValueError for anything the contract does not take"""
        if spec is None:
            return None
        from .components import check_connectivity
        from .reconstruct import check_h
        if not isinstance(spec, dict) or 'op' not in spec or not set(spec) <= {'op', 'h', 'connectivity'}:
            raise ValueError("geodesic is None or {'op', 'h', 'connectivity'}, not %r" % (spec,))
        h = check_h(spec['op'], spec['h'] if spec.get('h') is not None else 0, 65535)      # h is open above: an R8 volume takes min(h, 255)
        return {'op': spec['op'], 'h': h, 'connectivity': check_connectivity(spec['connectivity'] if spec.get('connectivity') is not None else 6)}

    @staticmethod
    def _combine_spec(spec):
        """the `combine` option with its defaults filled in, or None; raises ValueError for anything the contract does not take"""
        if spec is None:
            return None
        from .combine import check_op, check_channel, check_weights, check_mask
        from .resample import check_mode
        known = {'reader', 'volume', 'op', 'channel', 'lo', 'hi', 'fill', 'wa', 'wb', 'offset', 'resample'}
        if not isinstance(spec, dict) or 'op' not in spec or not set(spec) <= known or (spec.get('reader') is None) == (spec.get('volume') is None):
            raise ValueError("combine is None or {'reader' | 'volume', 'op', 'channel', 'lo', 'hi', 'fill', 'wa', 'wb', 'offset', 'resample'} with one "
                             "of 'reader' and 'volume', not %r" % (spec,))
        op = spec['op']
        check_op(op)
        if spec.get('volume') is not None and not isinstance(spec['volume'], Volume):
            raise ValueError("combine 'volume' is a Volume, not %r" % (spec['volume'],))
        out = {'reader': spec.get('reader'), 'volume': spec.get('volume'), 'op': op,
               'channel': check_channel(spec['channel'] if spec.get('channel') is not None else 0, 2), 'params': {}, 'resample': None}
        if spec.get('resample') is not None:
            check_mode(spec['resample'])
            out['resample'] = spec['resample']
        given = lambda keys: any(spec.get(k) is not None for k in keys)
        if op != 'mask' and given(('lo', 'hi', 'fill')):
            raise ValueError("combine 'lo', 'hi' and 'fill' go with op 'mask'")
        if op != 'blend' and given(('wa', 'wb', 'offset')):
            raise ValueError("combine 'wa', 'wb' and 'offset' go with op 'blend'")
        if op == 'mask':
            lo = spec['lo'] if spec.get('lo') is not None else 0
            fill = spec['fill'] if spec.get('fill') is not None else 0
            check_mask(lo, spec['hi'] if spec.get('hi') is not None else 65535, fill, 65535, 65535)
            out['params'] = {'lo': lo, 'hi': spec.get('hi'), 'fill': fill}           # hi None: the second volume's largest code
        elif op == 'blend':
            if spec.get('wa') is None or spec.get('wb') is None:
                raise ValueError("combine op 'blend' needs 'wa' and 'wb'")
            wa, wb, offset = check_weights(spec['wa'], spec['wb'], spec['offset'] if spec.get('offset') is not None else 0)
            out['params'] = {'wa': wa, 'wb': wb, 'offset': offset}
        return out

    @staticmethod
    def _resample_spec(spec):
        """the `resample` option with its defaults filled in, or None; raises ValueError for anything the contract does not take"""
        if spec is None:
            return None
        from .resample import check_mode, check_size, check_spacing
        if not isinstance(spec, dict) or not set(spec) <= {'size', 'spacing', 'pitch', 'mode'} or ('size' in spec) == ('spacing' in spec):
            raise ValueError("resample is None, {'size': [w, h, d], 'mode'} or {'spacing': [sx, sy, sz], 'pitch', 'mode'}, not %r" % (spec,))
        mode = spec['mode'] if spec.get('mode') is not None else 'filtered'
        check_mode(mode)
        out = {'size': None, 'spacing': None, 'pitch': None, 'mode': mode}
        if 'size' in spec:
            if spec.get('pitch') is not None:
                raise ValueError("resample 'pitch' goes with 'spacing'")
            size = spec['size']
            if isinstance(size, (str, bytes)) or not hasattr(size, '__len__') or len(size) != 3:
                raise ValueError('resample size is [w, h, d], not %r' % (size,))
            out['size'] = check_size(*size)
        else:
            out['spacing'], out['pitch'] = check_spacing(spec['spacing'], spec.get('pitch'))
        return out

    @staticmethod
    def _resample_takes(volume, mode):
        from . import _native as N
        fmt = volume.native_format()[0]
        if mode == 'filtered':
            return fmt in (N.FORMAT_R8, N.FORMAT_RG8, N.FORMAT_R16, N.FORMAT_RG16)
        return not N.FORMAT_RGB565 <= fmt <= N.FORMAT_RGB9_E5

    @staticmethod
    def _distance_spec(spec, name='distance'):
        """the `distance` option (or, under its name, the `thickness` option: seeds 'rest' and steps 2 by default) with its defaults filled
        in, or None; raises ValueError for anything the contract does not take"""
        if spec is None:
            return None
        from .distance import check_range, check_seeds, check_steps, check_within
        known = {'lo', 'hi', 'seeds', 'mode', 'from', 'to', 'fill', 'steps'}
        if not isinstance(spec, dict) or not {'lo', 'hi', 'mode'} <= set(spec) or not set(spec) <= known:
            raise ValueError("%s is None or {'lo', 'hi', 'seeds', 'mode': 'within' | 'channel', 'from', 'to', 'fill', 'steps'}, not %r" % (name, spec))
        if spec['mode'] not in ('within', 'channel'):
            raise ValueError("%s mode is 'within' or 'channel', not %r" % (name, spec['mode']))
        lo, hi = check_range(spec['lo'], spec['hi'], 65535)
        thickness = name == 'thickness'
        seeds = spec['seeds'] if spec.get('seeds') is not None else ('rest' if thickness else 'range')
        check_seeds(seeds)
        out = {'lo': lo, 'hi': hi, 'seeds': seeds, 'mode': spec['mode'], 'from': 0, 'to': None, 'fill': 0, 'steps': 2 if thickness else 1}
        if spec['mode'] == 'within':
            if spec.get('steps') is not None:
                raise ValueError("%s 'steps' goes with mode 'channel'" % name)
            r2_lo, r2_hi, fill = check_within(spec['from'] if spec.get('from') is not None else 0, spec.get('to'),
                                              spec['fill'] if spec.get('fill') is not None else 0, 65535)
            out.update({'from': r2_lo, 'to': r2_hi, 'fill': fill})
        else:
            if any(spec.get(k) is not None for k in ('from', 'to', 'fill')):
                raise ValueError("%s 'from', 'to' and 'fill' go with mode 'within'" % name)
            out['steps'] = check_steps(spec['steps'] if spec.get('steps') is not None else out['steps'])
        return out

    @staticmethod
    def _components_spec(spec):
        """the `components` option with its defaults filled in, or None; raises ValueError for anything the contract does not take"""
        if spec is None:
            return None
        from .components import check_connectivity, check_min_voxels, check_range, check_keep
        known = {'lo', 'hi', 'connectivity', 'minVoxels', 'mode', 'keep'}
        if not isinstance(spec, dict) or not {'lo', 'hi', 'mode'} <= set(spec) or not set(spec) <= known:
            raise ValueError("components is None or {'lo', 'hi', 'connectivity', 'minVoxels', 'mode': 'keep' | 'label', 'keep'}, not %r" % (spec,))
        if spec['mode'] not in ('keep', 'label'):
            raise ValueError("components mode is 'keep' or 'label', not %r" % (spec['mode'],))
        lo, hi = check_range(spec['lo'], spec['hi'], 65535)
        out = {'lo': lo, 'hi': hi, 'mode': spec['mode'],
               'connectivity': check_connectivity(spec['connectivity'] if spec.get('connectivity') is not None else 6),
               'minVoxels': check_min_voxels(spec['minVoxels'] if spec.get('minVoxels') is not None else 1), 'keep': None}
        if spec.get('keep') is not None:
            if spec['mode'] == 'label':
                raise ValueError("components 'keep' goes with mode 'keep'")
            out['keep'] = check_keep(1, spec['keep'], 0, 65535)[1]
        return out

    @staticmethod
    def _window_spec(window):
        """('values', lo, hi) | ('range',) | ('percentiles', a, b) of a `window` option; raises ValueError for anything else"""
        if window == 'range':
            return ('range',)
        if isinstance(window, dict) and set(window) == {'percentiles'} and len(window['percentiles']) == 2:
            a, b = (float(p) for p in window['percentiles'])
            if not 0 <= a <= b <= 100:
                raise ValueError('window percentiles %r: 0 <= a <= b <= 100' % (window['percentiles'],))
            return ('percentiles', a, b)
        if isinstance(window, (list, tuple)) and len(window) == 2 and not any(isinstance(x, (str, bool)) for x in window):
            return ('values', window[0], window[1])
        raise ValueError("window is None, [lo, hi], 'range' or {'percentiles': [a, b]}, not %r" % (window,))

    def _window_of(self, volume):
        """(lo, hi) of the `window` option for this volume"""
        from . import _native as N
        spec = self._window_spec(self.window)
        if spec[0] == 'values':
            return spec[1], spec[2]
        if spec[0] == 'percentiles':
            return volume.percentile_window(spec[1], spec[2])
        lo, hi = volume.range()
        if volume.native_format()[0] != N.FORMAT_R32F:
            hi = max(hi, lo + 1)
        return lo, hi

    @staticmethod
    def _one_channel_unorm(volume):
        from . import _native as N
        return volume.native_format()[0] in (N.FORMAT_R8, N.FORMAT_R16)

    def setEnvironmentMap(self, image):                                               # :135-140 — RGBA8, float [h][w][4] or read_hdr()'s
        self.environmentTexture = image
        if self.renderer:
            self.renderer.setEnvironmentMap(image)

    def setFilter(self, filter):                                                      # :142-150
        self.filter = filter
        if self.volume:
            self.volume.setFilter(filter)
            if self.renderer:
                self.renderer.reset()

    def chooseRenderer(self, renderer):                                               # :152-167
        if self.renderer:
            self.renderer.destroy()
        rendererClass = RendererFactory(renderer)
        options = {'resolution': self._resolution, 'transform': self.volumeTransform}
        if self._rng is not None:
            options['rng'] = self._rng
        self.renderer = rendererClass(self.gl, self.volume, self.camera, self.environmentTexture, options)
        self.renderer.reset()
        if self.toneMapper:
            self.toneMapper.setTexture(self.renderer)
        self.isTransformationDirty = True

    def chooseToneMapper(self, toneMapper):                                           # :169-188
        if self.toneMapper:
            self.toneMapper.destroy()
        toneMapperClass = ToneMapperFactory(toneMapper)
        self.toneMapper = toneMapperClass(self.gl, self.renderer, {'resolution': self._resolution})

    def render(self):                                                                 # :190-210
        if not self.renderer or not self.toneMapper:
            return
        self.renderer.render()
        self.toneMapper.render()

    def getFrame(self):
        """what the reference puts on the canvas: the tone mapper's RGBA8 image, read back"""
        return self.toneMapper.getTexture()

    def recordAnimationToImageSequence(self, options=None):
        """RenderingContext.js:259-305, headless and deterministic: for every frame time t = startTime + i / fps the camera
        animator is stepped, the renderer reset and `passes` render() calls made (the reference renders for `frameTime`
        seconds of wall clock instead), and the tone-mapped frame is written as directory/frame%04d.png.
        options: {'directory', 'startTime', 'endTime', 'fps', 'passes'}; dispatches 'animationprogress'."""
        import math
        import os
        from .png import write_png
        options = options or {}
        if self.cameraAnimator is None or not self.renderer or not self.toneMapper:
            raise RuntimeError('recordAnimationToImageSequence needs a cameraAnimator, a renderer and a tone mapper')
        directory = options['directory']
        startTime, endTime, fps = options.get('startTime', 0), options.get('endTime', 1), options.get('fps', 30)
        passes = int(options.get('passes', 16))
        frames = max(math.ceil((endTime - startTime) * fps), 1)                       # :261
        timeStep = 1 / fps
        os.makedirs(directory, exist_ok=True)
        files = []
        for i in range(frames):
            t = startTime + i * timeStep                                              # :283
            self.cameraAnimator.update(t)
            self.renderer.reset()                                                     # :286
            for _ in range(passes):
                self.render()
            path = os.path.join(directory, 'frame%s.png' % str(i).zfill(4))           # :291
            write_png(path, self.getFrame())
            files.append(path)
            self.dispatchEvent(CustomEvent('animationprogress', {'detail': (i + 1) / frames}))   # :298-300
        return files

    @property
    def resolution(self):                                                             # :212-214
        return self._resolution

    @resolution.setter
    def resolution(self, resolution):                                                 # :216-229
        self._resolution = resolution
        if self.renderer:
            self.renderer.setResolution(resolution)
        if self.toneMapper:
            self.toneMapper.setResolution(resolution)
            if self.renderer:
                self.toneMapper.setTexture(self.renderer)
