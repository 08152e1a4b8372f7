"""GPU: fixed-seed renderer lives (tests/renderer_life_cases.py) replayed on the device beside the CPU oracle.  A life is what one renderer
object goes through: passes of every form (render() fused and hook by hook, frame sequences, buckets into a frame ring, displayed
frames), resets, transfer functions, environment maps, matrices, properties, filter changes and uploads on the bound volume,
setVolume with another storage format, setResolution, every implementation option, redirected render targets, a tone mapper that comes
and goes, and reads in the middle — in an order nobody chose.  The oracle is the model and never reads device state: it gets the
uniforms the host object drew (a recording rng, the blocks _prepare_frame_uniforms handed out) and resets exactly when the host object
does (reset wrapped on the instance).

After every pass event and at every read: the current destination's RGBA16F image bit for bit (every slot of a frame sequence or bucket),
for half of the lives every state buffer as well, for the "lazy" half (seed % 4 in (1, 2)) the state after the last event only; sample_count() for unsharded
lives; a bound tone mapper's texture byte for byte against oracle.tonemap.  Every life is replayed a second time with every optional path
off (the plain twin: no tile classes, one stream, no atlas, records, persistent forms or fused tone mapping, option events ignored) and
must give the same buffers at every check point; fast-math MCM lives, which have no bit-exact CPU mirror, are held to their plain twin alone.

VPT_LIFE_SEEDS=a:b widens the sweep; VPT_LIFE_PREFIX=n replays only the first n events of every life (to bisect a failure by hand).

What the model had to learn from the library (include/vpt.h says each of them): the last slot of vpt_renderer_play_into stays the render
target; vpt_tonemapper_render reads the memory the renderer's frames go to, a redirected target included;
vpt_renderer_play_into_display wants the renderer's own buffer as the target and does not say what that buffer holds afterwards;
sample_count() counts through a resize."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.property_bag import CustomEvent
from vpt_amd.scene import Node, Transform
from vpt_amd.synthetic import GoldenRatioRng

import renderer_life_cases as L
from test_gpu_fuzz import same_bits, MCM_BUFFERS

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_LIFE_SEEDS", "%d:%d" % L.DEFAULT_SEEDS).split(":")])
_PREFIX = int(os.environ.get("VPT_LIFE_PREFIX", "-1"))
_BUFFER = {'position': N.BUFFER_MCM_POSITION, 'direction': N.BUFFER_MCM_DIRECTION, 'transmittance': N.BUFFER_MCM_TRANSMITTANCE,
           'radiance': N.BUFFER_MCM_RADIANCE, 'accum': N.BUFFER_ACCUM}


class RecordingRng:
    """GoldenRatioRng that keeps every value it hands out"""

    def __init__(self, start):
        self.inner, self.log = GoldenRatioRng(start), []

    def __call__(self):
        self.log.append(self.inner())
        return self.log[-1]


class OracleModel:
    """the CPU oracle as the model of a life; everything it answers goes onto `tape`, which a TapeModel hands out again in the same order
    (the plain twin asks the same questions: the oracle runs once per life)"""

    def __init__(self, oracle, kind, size, nthreads=1):
        self.oracle, self.kind, self.nthreads, self.tape = oracle, kind, nthreads, []
        self.osc = self.o = None
        self.resize(size)

    def resize(self, size):
        self.w, self.h = size
        samples = self.o.samples if self.o is not None else 0
        self.o = self.oracle.OracleRenderer(self.kind, self.osc, self.w, self.h)
        self.o.samples = samples                          # (sample_count() counts since the renderer's creation, through a resize)

    def scene(self, texels, filt, tf, env):
        self.osc = self.oracle.OracleScene(texels, filt, tf=tf, env=env)
        self.o.scene = self.osc                           # (the state arrays live in the OracleRenderer and survive)

    def lao(self, p):
        self.o.lao = self.oracle.lao_params(**p)

    def reset(self, m, seed):
        self.o.reset(self.oracle.make_frame(self.w, self.h, m, seed=seed) if seed is not None else self.oracle.make_frame(self.w, self.h, m))

    def render_pass(self, u):
        fr = self.oracle.make_frame(self.w, self.h, np.array(list(u.mvp_inverse), np.float32), nthreads=self.nthreads)
        fr.seed = u.rand_seed; fr.offset = u.offset; fr.step = u.step_size
        fr.extinction = u.extinction; fr.anisotropy = u.anisotropy; fr.max_bounces = u.max_bounces; fr.steps = u.steps
        for i in range(3):
            fr.light_dir[i] = u.light_direction[i]
        fr.mix = u.mix; fr.blur = u.blur
        fr.isovalue = u.isovalue; fr.gradient_step = u.gradient_step; fr.threshold = u.threshold
        self.o.render(fr)
        return self._out(self.o.out.copy())

    def state(self):
        return self._out([s.copy() for s in self.o.state] if self.kind == "mcm" else [self.o.acc.copy(), self.o.frame.copy()])

    def samples(self):
        return self._out(int(self.o.samples))

    def tonemap(self, kind, image, params):
        return self._out(self.oracle.tonemap(kind, image, **params))

    def _out(self, v):
        self.tape.append(v)
        return v


class TapeModel:
    """the answers an OracleModel gave, once more; a fast-math life has no model: tape None, every answer None"""

    def __init__(self, tape):
        self.tape = None if tape is None else list(tape)

    def resize(self, size): pass
    def scene(self, *a): pass
    def lao(self, p): pass
    def reset(self, m, seed): pass

    def _next(self, *a):
        return None if self.tape is None else self.tape.pop(0)

    render_pass = state = samples = tonemap = _next


def upload(ctx, fmt, texels, filt):
    if fmt == 'R8_SNORM':
        return vpt_amd.Volume.from_array(ctx, texels, filt, snorm=True)
    return vpt_amd.Volume.from_array(ctx, texels, filt, norm16=fmt in ('R16', 'R16_SNORM'))


class Replay:
    """one life on the device (ctx None, inside test_gpu_fuzz.oracle_only(): the host objects and the model alone) beside `model`"""

    def __init__(self, ctx, model, s, plain=False):
        self.ctx, self.model, self.s, self.plain, self.device = ctx, model, s, plain, ctx is not None
        self.kind = s.kind
        self.gots = []                                    # (label, array) of everything read from the device, in order
        self.r = self.tm = None
        self.tm_kind = None
        self.holders, self.gvols = [], [None] * len(s.volumes)
        self.nresets = 0
        self.watch, self.tile_classes = False, []         # watch: r.tile_classes() after every event (it joins the side streams: not by default)
        self.settled = []                                 # ... and MCM's settled_passes() before every event
        self.image = None                                 # the model's image of the last pass

    # ---- the pieces ----------------------------------------------------------------------------------------------------------------
    def what(self, i=None):
        return "%s\n%s%s" % (L.describe(self.kind, self.s.seed, self.s), "plain twin, " if self.plain else "", "before event 0" if i is None else "event %d" % i)

    def gvol(self, k):
        if self.device and self.gvols[k] is None:
            self.gvols[k] = upload(self.ctx, self.s.volumes[k][0], self.raw[k], self.filters[k])
        return self.gvols[k]

    def new_scene(self):
        fmt = self.s.volumes[self.bound][0]
        self.model.scene(L.decode(self.raw[self.bound], fmt).copy(), self.filters[self.bound], self.tf, self.env)

    def option(self, name, value):
        if self.device:
            self.r.set_option(L.OPTIONS[name][0] if isinstance(name, str) else name, value)

    def size(self):
        return self.r._size()

    def rows_of(self, img):
        """the local rows of a global [h][w][...] array, and which of them are no padding"""
        w, h = self.size()
        valid = self.rows >= 0
        return np.ascontiguousarray(img).reshape(h, -1)[self.rows[valid]], valid

    def check(self, got, want, label):
        """got (local rows) against the model's want (global rows; None: the model does not say, or a fast-math life has no model); what is
        kept for the comparison with the plain twin is the rows that are no padding, and only where a model or a fast-math twin decides"""
        got = np.ascontiguousarray(got).reshape(len(self.rows), -1)[self.rows >= 0]
        if want is not None or self.s.fast:
            self.gots.append((label, got.copy()))
        if want is not None:
            same_bits(got, self.rows_of(want)[0], label)

    def setup(self):
        s, kind = self.s, self.kind
        self.camera = L.build_camera(s.cam, s.aspect)
        self.transform = Transform(Node())
        L.set_model(self.transform, s.model)
        self.raw = [t.copy() for _, _, t in s.volumes]
        self.filters = [f for _, f, _ in s.volumes]
        self.bound, self.tf, self.env = 0, s.tf, s.env
        self.rng = RecordingRng(s.start)
        opts = {'resolution': s.size, 'transform': self.transform, 'rng': self.rng, 'fused': True}
        if s.shard:
            opts['shard'] = s.shard
        self.opts = opts
        r = self.r = vpt_amd.RendererFactory(kind)(self.ctx if self.device else types.SimpleNamespace(_h=None), self.gvol(0), self.camera, s.env, opts)
        if self.plain:
            self.option(N.OPTION_SPLIT_STREAMS, 1)
            if kind != 'lao':
                self.option(N.OPTION_TILE_CLASSES, 0)
            if kind == 'mcm':
                for o in (N.OPTION_SETTLED_MISS, N.OPTION_BOUNDARY_ATLAS, N.OPTION_COLUMN_RECORDS, N.OPTION_MCM_PERSISTENT):
                    self.option(o, 0)
            if kind == 'mcs':
                self.option(N.OPTION_MCS_PERSISTENT, 0)
        elif s.split:
            self.option(N.OPTION_SPLIT_STREAMS, s.split)
        if s.fast:
            self.option(N.OPTION_FAST_MATH, 1)
        self.rows = r.global_rows() if self.device else np.arange(s.size[1])
        self.mem = {'own': np.zeros(s.size[0] * s.size[1] * 4, np.uint16)}      # destination -> the image the model says it holds
        self.dest = 'own'
        self.frames = []                                  # the uniform blocks _prepare_frame_uniforms handed out
        self.last_hooks = False
        real_reset, real_prepare = r.reset, r._prepare_frame_uniforms

        def reset():                                      # the model resets exactly when the host object does
            n0 = len(self.rng.log)
            real_reset()
            seed = None
            if kind == 'mcm':                              # MCMRenderer.js:93: the reset's own draw
                assert len(self.rng.log) == n0 + 1
                seed = np.float32(self.rng.log[n0])
            self.model.reset(r._matrix(), seed)
            self.nresets += 1

        def prepare():
            u = real_prepare()
            self.frames.append(N.Uniforms.from_buffer_copy(u))
            return u
        r.reset, r._prepare_frame_uniforms = reset, prepare
        self.new_scene()
        if s.tf is not None:
            r.setTransferFunction(s.tf)
        for name, value in s.props.items():
            setattr(r, name, value)
        r.reset()

    def ring_holders(self):
        """two idle renderers of the life's size and shard: their render buffers are the redirected targets, the first one's frame ring the
        bucket memory (tests/test_gpu_mcm_settled.py test_destinations)"""
        if not self.holders and self.device:
            for _ in range(2):
                opts = dict(self.opts, resolution=self.size(), rng=GoldenRatioRng())
                self.holders.append(vpt_amd.MCMRenderer(self.ctx, self.gvol(0), L.build_camera(self.s.cam, self.s.aspect), None, opts))
            self.fill_ring()
        return self.holders

    def fill_ring(self):
        h = self.holders[0]
        h.reset(); h.play(16, frames=True)                 # VPT_FRAME_SLOTS: allocates the ring

    def ring(self):
        p, n = C.c_void_p(), C.c_size_t()
        N.check(N.lib().vpt_renderer_frame_ring_device(self.ring_holders()[0]._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def read_dest(self):
        r = self.r
        if self.dest == 'own':
            return r.getTexture().view(np.uint16)
        r.join(); self.ctx.synchronize()
        if self.dest[0] == 'holder':
            return self.holders[self.dest[1]].getTexture().view(np.uint16)
        return self.holders[0].read_frame_slot(self.dest[1]).view(np.uint16)

    def tm_params(self):
        return {p['name']: getattr(self.tm, p['name']) for p in self.tm.properties}

    def check_tm(self, label):
        self.tm.render()
        if self.dest not in self.mem:                      # (behind play_into_display the model does not say what the own buffer holds)
            return
        got = self.tm.getTexture()
        own = self.mem[self.dest]                          # (vpt_tonemapper_render reads where the renderer's frames go: a redirected target too)
        w, h = self.size()
        want = self.model.tonemap(self.tm_kind, None if own is None else own.view(np.float16).reshape(h, w, 4), self.tm_params())
        self.check(got, want, label + ": the tone mapper's texture")

    # ---- passes ----------------------------------------------------------------------------------------------------------------------
    def lao(self):
        if self.kind == 'lao':
            r = self.r
            self.model.lao(dict(local_ambient_occlusion=int(r.localAmbientOcclusion), lao_weight=r.LAOWeight, num_lao_samples=r.numLAOSamples,
                                lao_step_size=r.LAOStepSize, soft_shadows=int(r.softShadows), shadows_weight=r.shadowsWeight,
                                num_shadow_samples=r.numShadowSamples, light_radius=r.lightRadious, light_coefficient=r.lightCoeficient,
                                light_position=r.lightPosition))

    def sequence(self, call, n):
        """the uniform blocks of the n passes `call` enqueues: what _prepare_frame_uniforms handed out, or (MCM's _collect_frames draws its
        seeds directly) the block of the first pass with the logged draws"""
        self.frames, n0 = [], len(self.rng.log)
        call()
        if self.kind != 'mcm':
            assert len(self.frames) == n
            return self.frames
        seeds = self.rng.log[n0:]
        assert len(seeds) == n
        us = []
        for sd in seeds:
            u = N.Uniforms.from_buffer_copy(self.r._u)
            u.rand_seed = float(np.float32(sd))
            us.append(u)
        return us

    def passes(self, e, label):
        r, n, op = self.r, e['n'], e['op']
        self.lao()
        images = []
        if op == 'render':
            for _ in range(n):
                r.render()
                images.append(self.model.render_pass(r._u))
            self.last_hooks = not r.fused
            self.mem[self.dest] = images[-1]
        elif op == 'play':
            mode = e['mode']
            us = self.sequence(lambda: r.play(n, use_graph=mode == 'graph', fused=mode == 'fused', frames=mode == 'frames'), n)
            images = [self.model.render_pass(u) for u in us]
            self.last_hooks = False
            self.mem[self.dest] = images[-1]
            if mode == 'frames' and self.device:
                for k in range(n):
                    self.check(r.read_frame_slot(k).view(np.uint16), images[k], "%s: frame slot %d" % (label, k))
        elif op == 'play_into':
            if self.kind == 'mcm':
                self.option(N.OPTION_BUCKET_KERNEL, 0 if self.plain else e['bucket'])
            ptr, slot = self.ring() if self.device else (1, 0)
            us = self.sequence(lambda: r.play_into(n, ptr, slot), n)
            images = [self.model.render_pass(u) for u in us]
            self.last_hooks = False
            for k in range(n):
                self.mem[('slot', k)] = images[k]
            self.dest = ('slot', n - 1)                  # (include/vpt.h: the last target stays the renderer's render target)
            if self.device:
                r.join(); self.ctx.synchronize()
                for k in range(n - 1):
                    self.check(self.holders[0].read_frame_slot(k).view(np.uint16), images[k], "%s: bucket slot %d" % (label, k))
        else:                                             # play_into_display: the frames as the armed tone mapper shows them, RGBA8
            w, h = self.size()
            self.dest = 'own'                             # (refused while a caller's render target is set)
            if self.device:
                r.set_render_target(None, 0)
                self.tm.set_option(N.TONEMAPPER_OPTION_TABLE, N.TONEMAPPER_TABLE_ALWAYS)
                self.tm.set_option(N.TONEMAPPER_OPTION_FUSE, 1)
                self.tm.render()
            ptr, _ = self.ring() if self.device else (1, 0)
            stride = w * len(self.rows) * 4
            us = self.sequence(lambda: r.play_into_display(self.tm if self.device else types.SimpleNamespace(_h=None), n, ptr, stride), n)
            images = [self.model.render_pass(u) for u in us]
            self.last_hooks = False
            params = self.tm_params() if self.device else {}
            for k in range(n):
                want = self.model.tonemap(self.tm_kind, None if images[k] is None else images[k].view(np.float16).reshape(h, w, 4), params) if self.device else None
                if self.device:
                    r.join(); self.ctx.synchronize()
                    pair = self.holders[0].read_frame_slot(k // 2).view(np.uint8).reshape(2, len(self.rows), w, 4)
                    self.check(pair[k % 2], want, "%s: displayed frame %d" % (label, k))
            self.mem = {k: v for k, v in self.mem.items() if k != 'own' and k[0] != 'slot'}      # the ring holds bytes now; the own buffer: either
            if self.device:
                r.set_render_target(None, 0)
                if self.plain:
                    self.tm.set_option(N.TONEMAPPER_OPTION_FUSE, 0)
            self.dest = 'own'
            self.image = images[-1]
            return
        self.image = images[-1]
        if self.device:
            self.check(self.read_dest(), images[-1], "%s: the image" % label)
            if not self.s.lazy:
                self.check_state(label)

    def check_state(self, label):
        r, want = self.r, self.model.state()
        if self.kind == 'mcm':
            for k, b in enumerate(MCM_BUFFERS):
                self.check(r.read(b), None if want is None else want[k], "%s: state buffer %d" % (label, b))
        else:
            self.check(r.read(N.BUFFER_ACCUM), None if want is None else want[0], "%s: the accumulation buffer" % label)
            if self.last_hooks:
                self.check(r.read(N.BUFFER_FRAME), None if want is None else want[1], "%s: the frame buffer" % label)

    def check_samples(self, label):
        want = self.model.samples()
        if self.device and not self.s.shard:
            got = self.r.sample_count()
            self.gots.append((label + ": samples", np.array([got], np.uint64)))
            assert want is None or got == want, "%s: sample_count() %d, the oracle %d" % (label, got, want)

    # ---- the other events --------------------------------------------------------------------------------------------------------------
    def event(self, e, label):
        r, op, dev = self.r, e['op'], self.device
        if op in L.PASS_OPS:
            self.passes(e, label)
        elif op == 'reset':
            r.reset()
        elif op == 'camera':
            L.move_camera(self.camera, e['cam'])
            if e['reset']:
                r.reset()
        elif op == 'transform':
            L.set_model(self.transform, e['model'])
        elif op == 'lens':
            L.set_lens(self.camera, e)
        elif op == 'fused':
            r.fused = e['value']
        elif op == 'tf':
            self.tf = e['tf']
            self.new_scene()
            if e['via'] == 'direct':
                r.setTransferFunction(e['tf'])
            else:
                r.transferFunction = e['tf']
                r.dispatchEvent(CustomEvent('change', {'detail': {'name': 'transferFunction', 'value': e['tf']}}))
        elif op == 'env':
            self.env = e['env']
            self.new_scene()
            r.setEnvironmentMap(e['env'])
        elif op == 'prop':
            setattr(r, e['name'], e['value'])
            r.dispatchEvent(CustomEvent('change', {'detail': {'name': e['name'], 'value': e['value']}}))
        elif op == 'filter':
            self.filters[e['vol']] = e['filter']
            if self.gvols[e['vol']] is not None:
                self.gvols[e['vol']].setFilter(e['filter'])
            self.new_scene()
        elif op == 'upload':
            x, y, z = e['at']
            b = e['block']
            self.raw[e['vol']][z:z + b.shape[0], y:y + b.shape[1], x:x + b.shape[2]] = b
            if self.gvols[e['vol']] is not None:
                self.gvols[e['vol']].upload_block(x, y, z, b)
            self.new_scene()
        elif op == 'wide':
            if self.gvols[e['vol']] is not None and not self.plain:
                self.gvols[e['vol']].set_wide_tables(e['value'])
        elif op == 'set_volume':
            self.bound = e['vol']
            self.new_scene()
            r.setVolume(self.gvol(self.bound))
        elif op == 'resize':
            if dev:
                r.set_render_target(None, 0)
            self.model.resize(e['size'])                   # (a new OracleRenderer, before setResolution's reset reaches the model)
            self.new_scene()
            r.setResolution(e['size'])
            self.rows = r.global_rows() if dev else np.arange(e['size'][1])
            for h in self.holders:
                h.setResolution(e['size'])
            if self.holders:
                self.fill_ring()
            if self.tm is not None:                        # RenderingContext.resize: the tone mapper follows and is bound again
                self.tm.setResolution(e['size'])
                self.tm.setTexture(r)
            self.mem, self.dest = {'own': np.zeros(e['size'][0] * e['size'][1] * 4, np.uint16)}, 'own'
        elif op == 'option':
            if not self.plain:
                self.option(e['option'], e['value'])
        elif op == 'target':
            if dev:
                if e['to'] is None:
                    r.set_render_target(None, 0)
                else:
                    r.set_render_target(*self.ring_holders()[e['to']].render_buffer_device())
            self.dest = 'own' if e['to'] is None else ('holder', e['to'])
        elif op == 'tm_create':
            if dev:
                if self.tm is not None:
                    self.tm.destroy()
                self.tm = vpt_amd.ToneMapperFactory(e['kind'])(self.ctx, r, {'resolution': self.size()})
                if self.plain:
                    self.tm.set_option(N.TONEMAPPER_OPTION_FUSE, 0)
            self.tm_kind = e['kind']
        elif op == 'tm_render':
            if dev:
                self.check_tm(label)
        elif op == 'tm_params':
            if dev:
                for k, v in e['values'].items():
                    setattr(self.tm, k, v)
        elif op == 'tm_option':
            if dev and e['option'] == 'table':
                self.tm.set_option(N.TONEMAPPER_OPTION_TABLE, e['value'])
            elif dev and not self.plain:
                self.tm.set_option(N.TONEMAPPER_OPTION_FUSE, e['value'])
        elif op == 'tm_destroy':
            if dev:
                self.tm.destroy()
            self.tm = self.tm_kind = None
        elif op == 'read':
            if dev:
                for again in range(2 if e['twice'] else 1):
                    for b in e['buffers']:
                        what = "%s: %s%s" % (label, b, ", read again" if again else "")
                        if b == 'render':
                            if self.dest in self.mem:
                                self.check(self.read_dest(), self.mem[self.dest], what)
                        else:
                            want = self.model.state()
                            self.check(r.read(_BUFFER[b]), None if want is None else want[MCM_BUFFERS.index(_BUFFER[b]) if self.kind == 'mcm' else 0], what)
        elif op == 'sample_count':
            self.check_samples(label)
        else:
            raise KeyError(op)

    def run(self):
        s = self.s
        events = s.events if _PREFIX < 0 else s.events[:_PREFIX]
        try:
            self.setup()
            expected = 1
            for i, e in enumerate(events):
                if self.watch and self.kind == 'mcm':
                    self.settled.append(self.r.settled_passes())
                self.event(e, self.what(i))
                if self.watch:
                    self.tile_classes.append(self.r.tile_classes())
                expected += L.resets_of(self.kind, e)
                assert self.nresets == expected, "%s: %d resets so far, the cases module expects %d" % (self.what(i), self.nresets, expected)
            if self.device:
                if self.dest in self.mem:
                    self.check(self.read_dest(), self.mem[self.dest], self.what(len(events)) + " (the end): the image")
                self.check_state(self.what(len(events)) + " (the end)")
            self.check_samples(self.what(len(events)) + " (the end)")
            if self.device and _PREFIX < 0:
                self.early()
        finally:
            self.close()
        return self

    def early(self):
        """one life in four destroys the bound volume or the tone mapper BEFORE the renderer: both must end cleanly"""
        if self.s.early == 'volume':
            u = self.r._prepare_frame_uniforms()
            vol = self.gvols[self.bound]
            N.check(N.lib().vpt_volume_destroy(vol.texture))          # behind the host mirror's back (test_renderer_survives_its_volume)
            vol.texture = None; vol.ready = False
            rc = N.lib().vpt_renderer_render(self.r._h, C.byref(u))
            assert rc == -3 and b"no ready volume" in N.lib().vpt_last_error(), (rc, N.lib().vpt_last_error())
        elif self.s.early == 'tonemapper':
            if self.tm is None:                            # (a life that ends without one binds one first)
                self.event({'op': 'tm_create', 'kind': 'range'}, "a tone mapper to destroy early")
                self.tm.render()
            self.tm.destroy(); self.tm = self.tm_kind = None
            self.passes({'op': 'render', 'n': 1}, self.what(len(self.s.events)) + ", a pass after the tone mapper has gone")

    def close(self):
        if not self.device:
            return
        for x in [self.r, self.tm] + self.holders + self.gvols:
            if x is not None:
                x.destroy()
        self.r = self.tm = None
        self.holders, self.gvols = [], []


def oracle_side(oracle, s, nthreads=1):
    """the model's side of a life alone (inside test_gpu_fuzz.oracle_only()): the Replay, whose .image is the last pass's image"""
    return Replay(None, OracleModel(oracle, s.kind, s.size, nthreads), s).run()


def both_replays(gpu_ctx, oracle, s):
    model = TapeModel(None) if s.fast else OracleModel(oracle, s.kind, s.size)
    drawn = Replay(gpu_ctx, model, s).run()
    plain = Replay(gpu_ctx, TapeModel(model.tape), s, plain=True).run()
    assert len(drawn.gots) == len(plain.gots)
    for (la, a), (lb, b) in zip(drawn.gots, plain.gots):      # (a bit-exact life's replays both equal the oracle already)
        same_bits(a, b, "the drawn replay against its plain twin, " + la)
    return drawn


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", L.KINDS)
@pytest.mark.parametrize("seed", _SEEDS)
def test_life(gpu_ctx, oracle, kind, seed):
    both_replays(gpu_ctx, oracle, L.setup(kind, seed))


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", L.KINDS)
def test_the_lives_engage_the_tile_classes(gpu_ctx, oracle, kind):
    """checks that only met the general kernels would be vacuous: the first three default seeds in the armed position see both tile
    classes after a reset (LAO has no tile classes: its lives are held to the oracle alone), and MCM settles in at least one of them"""
    seeds = L.engaging_seeds(kind)
    assert len(seeds) == 3, seeds
    settled = 0
    for seed in seeds:
        s = L.setup(kind, seed)
        rep = Replay(gpu_ctx, TapeModel(None) if s.fast else OracleModel(oracle, kind, s.size), s)
        passes = []
        rep.watch = True
        real_close = rep.close
        rep.close = lambda: (passes.append(rep.r.settled_passes() if kind == 'mcm' else 0), real_close())
        rep.run()
        settled += passes[0]
        if kind != 'lao':
            assert any(hit > 0 and miss > 0 for hit, miss, _ in rep.tile_classes), (kind, seed, rep.tile_classes)
        assert all(v == 0 for _, _, v in rep.tile_classes), (kind, seed, rep.tile_classes)
    if kind == 'mcm':
        assert settled > 0, seeds


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_a_float_map_arrives_while_settled_samples_are_owed(gpu_ctx, oracle):
    """the default MCM lives the cases module names (owed()) do reach vpt_renderer_set_environment_texels with samples of the settled MISS
    kernel outstanding: the pass event right before the map ran that kernel, and the life holds no read in between"""
    seeds = [seed for seed in range(*L.DEFAULT_SEEDS) if L.owed('mcm', seed) is not None]
    assert len(seeds) >= 2, seeds
    for seed in seeds:
        s = L.setup('mcm', seed)
        rep = Replay(gpu_ctx, OracleModel(oracle, 'mcm', s.size), s)
        rep.watch = True
        rep.run()
        at = L.owed('mcm', seed)
        assert rep.settled[at] > rep.settled[at - 1], (seed, at, rep.settled)
