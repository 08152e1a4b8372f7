#!/usr/bin/env python3
"""Worker of tests/test_gpu_stream_order.py (a fresh process: torch's GPU state stays out of the pytest process; one GPU).

vpt_context_create_on_stream promises that the library's work orders with the caller's other work on that stream without host
synchronisation, and VPT_OPTION_SPLIT_STREAMS that callers see the usual in-order semantics although passes run on private side
streams.  Every scenario of SCENARIOS runs on a context built on a non-default torch.cuda.Stream, three times on the same inputs:

  twin     torch.cuda.synchronize() and ctx.synchronize() follow every step: what the calls compute when nothing overlaps.
  stale    the twin run without the producer: the source tensors keep their stale pattern (zeros).  Its result must differ from the
           twin's in at least STALE_FRACTION of the bytes, or the scenario could not tell fresh inputs from stale ones.
  ordered  no host synchronisation of the worker's own.  A delay kernel (the gate, torch.cuda._sleep) sits at the head of the stream
           with a torch event behind it; then, on the stream: torch kernels that write the source tensors (the producer), the
           library calls, and a torch copy of the result (the consumer; library-owned memory through a __cuda_array_interface__ view,
           never a host read).  Its bytes must equal the twin's.  In a scenario marked asynchronous the gate event must still be
           pending when the last library call has returned: none of its entries waited for the host.  A scenario that contains an
           entry of BLOCKING_ENTRIES is marked blocking: the gate stands in front of that call and only the bytes are asserted.

One line per scenario:  RESULT <tab> name <tab> PASS | FAIL | ERROR <tab> json.  After any exception (a HIP error among them) the
worker stops, runs no further scenario and exits non-zero.  Exit code 0 = every scenario passed.

The scenario table is plain data and importing this module touches no GPU (tests/test_stream_order_cases.py reads it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H = 208, 144                  # 13 x 9 tiles: three tile-row ranges of three rows, HIT and MISS tiles under CAMERA
CAMERA = (0.7, -0.3, 3.2)        # yaw, pitch, distance of the orbiting camera: far enough that most tiles miss the cube
PASSES = 3
STALE_FRACTION = 0.01
# The gate.  Measured on an MI355X with the library of the commit before these tests: torch.cuda._sleep runs GATE_MS_PER_CYCLE
# milliseconds per cycle, and the asynchronous scenario that takes the host longest to enqueue (LONGEST_ENQUEUE_MS, gate() to the
# return of its last library call) is named in DESIGN.md section 6.  The gate is at least ten times that, so that a loaded host still
# finds it closed, and stays under half a second, so that nothing looks like a hang.
GATE_MS_PER_CYCLE = 4.185e-7     # 4.185 ms for 10^7 cycles, 0.425 ms for 10^6
LONGEST_ENQUEUE_MS = 0.402       # C_chain; the others 0.09 .. 0.35 ms
GATE_CYCLES = 60000000           # 25 ms: 62 times the longest enqueue
# The caller's other work takes its time too: in the ordered run a short delay kernel (2 ms) stands where a scenario says lag(), between
# two library calls.  A side stream that failed to wait for the context's stream then runs well ahead of it, not a few microseconds.
LAG_CYCLES = 5000000

# what a scenario may call between the gate and its last library call, by the name its `entries` list uses
ASYNC_ENTRIES = (
    'upload_block_device', 'finalize', 'reduce', 'smooth(1)', 'rank(1)', 'combine', 'window', 'derive_gradient', 'resample(nearest)',
    'reset', 'render', 'play(fused)', 'play(frames)', 'play_into', 'play_into_display', 'set_render_target', 'join', 'setVolume',
    'setFilter', 'set_option', 'render_buffer_device', 'frame_ring_device', 'tonemapper.render', 'tonemapper.output_device',
    'graph.classes', 'graph.branch_components', 'label',
)
BLOCKING_ENTRIES = (
    'upload_block', 'setTransferFunction', 'set_environment', 'set_environment_texels', 'finalize(float)', 'smooth(n)', 'rank(n)',
    'resample(filtered)', 'components', 'keep', 'distance', 'channel', 'graph', 'graph.prune', 'read', 'resize', 'destroy', 'context.destroy',
)
FAMILIES = {
    'A': 'producer -> upload_block_device -> passes -> consumer',
    'B': 're-upload under passes in flight',
    'C': 'derived volumes',
    'D': 'tables changed between split passes',
    'E': 'tone mapper',
    'F': 'buckets and frame sequences',
    'G': 'lifetime on a caller\'s stream',
}
DIMS = {'r8': (20, 24, 28), 'r16': (23, 25, 29), 'rgb565': (22, 24, 28)}      # width, height, depth
SPLIT = {'mip': 3, 'eam': 3, 'depth': 3, 'mcs': 2, 'mcm': 2}                  # the library's stream counts for a 1080p frame, asked for here


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness one run of a scenario sees
# ---------------------------------------------------------------------------------------------------------------------------------
class Env:
    """what every run shares: the modules, the device, the torch stream and the context built on it"""


class Harness:
    def __init__(self, env, mode):
        self.env, self.mode, self.ctx = env, mode, env.ctx
        self.after_gate = False
        self.used, self.calls = set(), []
        self.outputs, self.owned, self.targets, self.checks = [], [], [], []
        self.gate_pending, self.enqueue_ms, self.gate_ms = None, None, None
        self._g0 = self._g1 = None
        self._t_gate = 0.0

    # ---- ordering -------------------------------------------------------------------------------------------------------------
    def step(self):
        if self.mode != 'ordered':
            self.env.torch.cuda.synchronize()
            if self.ctx is not None:
                self.ctx.synchronize()

    def do(self, entry, fn, *args, **kwargs):
        """one library call, under the name the scenario's `entries` list gives it"""
        t0 = time.perf_counter()
        out = fn(*args, **kwargs)
        if self.after_gate:
            self.used.add(entry)
            self.calls.append((entry, (time.perf_counter() - t0) * 1e3))
        self.step()
        return out

    def gate(self):
        """everything before this call is done and synchronised; in the ordered run the delay kernel and its event go in here"""
        torch = self.env.torch
        torch.cuda.synchronize()
        if self.ctx is not None:
            self.ctx.synchronize()
        if self.mode == 'ordered':
            self._g0, self._g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self._g0.record()
            torch.cuda._sleep(self.env.gate_cycles)
            self._g1.record()
        self.after_gate = True
        self._t_gate = time.perf_counter()

    def lag(self):
        """slow work of the caller's on the stream (ordered run)"""
        if self.mode == 'ordered':
            self.env.torch.cuda._sleep(LAG_CYCLES)

    def closed(self):
        """right behind the last library call: is the gate still closed?"""
        if self.mode == 'ordered':
            self.gate_pending = not self._g1.query()
            self.enqueue_ms = (time.perf_counter() - self._t_gate) * 1e3

    # ---- the caller's own work on the stream ------------------------------------------------------------------------------------
    def source(self, array):
        """(source tensor holding the stale pattern, device copy of `array` the producer writes into it); before the gate"""
        np, torch = self.env.np, self.env.torch
        array = np.ascontiguousarray(array)
        if array.dtype == np.uint16:
            array = array.view(np.int16)
        elif array.dtype == np.uint32:
            array = array.view(np.int32)
        data = torch.from_numpy(array).to(self.env.dev)
        return torch.zeros_like(data), data

    def produce(self, src, data):
        if self.mode != 'stale':
            self.env.torch.add(data, 0, out=src)
        self.step()

    def zeros(self, shape, dtype):
        return self.env.torch.zeros(shape, dtype=dtype, device=self.env.dev)

    def torch_op(self, fn, *args):
        out = fn(*args)
        self.step()
        return out

    def view(self, ptr, nbytes):
        """library-owned device memory as a torch tensor of bytes"""
        class DeviceBytes:
            __cuda_array_interface__ = {'shape': (int(nbytes),), 'typestr': '|u1', 'data': (int(ptr), False), 'version': 2}
        return self.env.torch.as_tensor(DeviceBytes(), device=self.env.dev)

    def take(self, tensor):
        """the consumer: a torch copy on the stream, straight behind the library's work"""
        self.outputs.append(tensor.clone())
        self.step()

    def check(self, what, fn):
        """a property of the outputs (list of uint8 arrays) beyond their equality; judged in the twin and the ordered run"""
        self.checks.append((what, fn))

    # ---- objects (all made before the gate unless the scenario says otherwise) ---------------------------------------------------
    def own(self, obj):
        self.owned.append(obj)
        return obj

    def noise(self, fmt, seed, dims=None):
        np = self.env.np
        w, h, d = dims or DIMS[fmt]
        rng = np.random.default_rng(seed)
        if fmt == 'r8':
            return rng.integers(0, 256, size=(d, h, w), dtype=np.uint16).astype(np.uint8)
        return rng.integers(0, 65536, size=(d, h, w), dtype=np.uint32).astype(np.uint16)

    def volume(self, fmt, array=None, dims=None):
        """a ready volume of `array`'s texels, uploaded from the host; None: the stale pattern"""
        import ctypes as C
        env, np, N = self.env, self.env.np, self.env.N
        w, h, d = dims or DIMS[fmt]
        if array is None:
            array = np.zeros((d, h, w), np.uint8 if fmt == 'r8' else np.uint16)
        if fmt == 'r8':
            return self.own(env.vpt.Volume.from_array(self.ctx, array, 'linear'))
        if fmt == 'r16':
            return self.own(env.vpt.Volume.from_array(self.ctx, array, 'linear', norm16=True))
        L, hnd = N.lib(), C.c_void_p()
        N.check(L.vpt_volume_create(self.ctx._h, w, h, d, N.FORMAT_RGB565, C.byref(hnd)))
        vol = env.vpt.Volume(self.ctx)
        vol.texture = hnd
        self.own(vol)
        N.check(L.vpt_volume_upload_block(hnd, 0, 0, 0, w, h, d, array.ctypes.data_as(C.c_void_p), array.nbytes))
        N.check(L.vpt_volume_finalize(hnd))
        vol.ready = True
        vol.setFilter('linear')
        return vol

    def renderer(self, kind, vol, split=None, size=(W, H), white=False):
        """white: MCM under the default 1 x 1 white environment, whose MISS tiles settle (their texels stop depending on the passes).  Otherwise
        MCM gets a float map, so that what its MISS-tile kernel computes on the side stream shows in the frame."""
        env, N, np = self.env, self.env.N, self.env.np
        texels = None
        if kind == 'mcm' and not white:
            texels = (np.random.default_rng(5).random((4, 8, 4), dtype=np.float32) * 1.5).astype(np.float32)
            texels[..., 3] = 1.0
        cls = {'mip': env.vpt.MIPRenderer, 'eam': env.vpt.EAMRenderer, 'mcs': env.vpt.MCSRenderer, 'mcm': env.vpt.MCMRenderer,
               'depth': env.vpt.DepthRenderer}[kind]
        r = cls(self.ctx, vol, orbit_camera(env, size[0] / size[1], *CAMERA), texels,
                {'resolution': size, 'transform': env.scene.Transform(env.scene.Node()), 'rng': env.synthetic.GoldenRatioRng()})
        self.own(r)
        r.set_option(N.OPTION_SPLIT_STREAMS, split or SPLIT[kind])
        if kind == 'mcm':
            r.set_option(N.OPTION_COLUMN_RECORDS, 1)       # (where the volume's format has them: one-channel bytes)
            r.extinction = 40
        if kind == 'mcs':
            r.extinction = 20
        return r

    def warm(self, r, passes=2):
        """split passes before the gate: the side streams exist and the lazy allocations are done"""
        r.reset()
        for _ in range(passes):
            r.render()

    def tonemapper(self, r, table, fuse, size=(W, H)):
        env, N = self.env, self.env.N
        tm = self.own(env.vpt.ReinhardToneMapper(self.ctx, r, {'resolution': size}))
        tm.exposure = 0.8
        tm.set_option(N.TONEMAPPER_OPTION_TABLE, N.TONEMAPPER_TABLE_ALWAYS if table else N.TONEMAPPER_TABLE_NEVER)
        tm.set_option(N.TONEMAPPER_OPTION_FUSE, 1 if fuse else 0)
        return tm

    def target(self, r, size=(W, H)):
        """a caller-owned render target for r (set by the scenario behind the gate)"""
        t = self.zeros((size[1], size[0], 4), self.env.torch.float16)
        self.targets.append(r)
        return t

    def finish(self):
        """the end of a run: drain, fetch the consumer's copies, let go of everything"""
        torch = self.env.torch
        torch.cuda.synchronize()
        if self.ctx is not None:
            self.ctx.synchronize()
        if self._g1 is not None:
            self.gate_ms = self._g0.elapsed_time(self._g1)
        outs = [o.contiguous().reshape(-1).view(torch.uint8).cpu().numpy() for o in self.outputs]
        self.outputs = []
        for r in self.targets:
            if r._h:
                r.set_render_target(0, 0)
        for obj in reversed(self.owned):
            obj.destroy()
        self.owned = []
        torch.cuda.synchronize()
        return outs


def orbit_camera(env, aspect, yaw, pitch, dist):
    """camera orbiting the cube centre (non-axis-aligned rays: all three slab axes)"""
    import math
    scene = env.scene
    node = scene.Node()
    qy = scene.quat.setAxisAngle(scene.quat.create(), [0, 1, 0], yaw)
    qx = scene.quat.setAxisAngle(scene.quat.create(), [1, 0, 0], pitch)
    node.transform.localRotation = scene.quat.multiply(scene.quat.create(), qy, qx)
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    node.transform.localTranslation = [dist * sy * cp, -dist * sp, dist * cy * cp]
    cam = scene.PerspectiveCamera(node)
    cam.aspect = aspect
    node.components.append(cam)
    return node


# ---------------------------------------------------------------------------------------------------------------------------------
# pieces the scenarios share
# ---------------------------------------------------------------------------------------------------------------------------------
def boxes(path, w, h, d):
    """the blocks of one whole-volume upload: 'slab' = full x-y extents (a device-to-device copy), 'box' = partial x-y extents (the
    blit kernel; a packed format: the decode kernel)"""
    if path == 'slab':
        return [(0, 0, 0, w, h, d // 2), (0, 0, d // 2, w, h, d - d // 2)]
    return [(0, 0, 0, 9, h, d), (9, 0, 0, w - 9, 11, d), (9, 11, 0, w - 9, h - 11, d)]


def sources(h, texels, blocks):
    out = []
    for (x, y, z, bw, bh, bd) in blocks:
        src, data = h.source(texels[z:z + bd, y:y + bh, x:x + bw])
        out.append(((x, y, z, bw, bh, bd), src, data))
    return out


def produce_and_upload(h, vol, blocks, finalize='finalize'):
    """finalize: the name of an explicit vpt_volume_finalize behind the uploads; None: left to the next pass that samples the volume"""
    N = h.env.N
    for _, src, data in blocks:
        h.produce(src, data)
    for (x, y, z, bw, bh, bd), src, _ in blocks:
        h.do('upload_block_device', vol.upload_block_device, x, y, z, bw, bh, bd, src.data_ptr(), src.numel() * src.element_size())
    if finalize:
        h.do(finalize, lambda: N.check(N.lib().vpt_volume_finalize(vol.texture)))


def own_frame(h, r):
    """the renderer's own render buffer behind its split passes"""
    h.do('join', r.join)
    ptr, nbytes = h.do('render_buffer_device', r.render_buffer_device)
    return h.view(ptr, nbytes)


def passes(h, r, n=PASSES):
    for _ in range(n):
        h.do('render', r.render)


def bytes_of(h, t):
    return t.numel() * t.element_size()


# ---------------------------------------------------------------------------------------------------------------------------------
# A. producer -> upload_block_device -> passes -> consumer
# ---------------------------------------------------------------------------------------------------------------------------------
def sc_upload(h, path, fmt, kind, target):
    w, hh, d = DIMS[fmt]
    vol = h.volume(fmt)
    r = h.renderer(kind, vol)
    h.warm(r)
    blocks = sources(h, h.noise(fmt, 11), boxes(path, w, hh, d))
    tgt = h.target(r) if target == 'caller' else None
    h.gate()
    produce_and_upload(h, vol, blocks, 'finalize(float)' if fmt == 'rgb565' else 'finalize')
    if tgt is not None:
        h.do('set_render_target', r.set_render_target, tgt.data_ptr(), bytes_of(h, tgt))
    h.do('reset', r.reset)
    passes(h, r)
    out = tgt if tgt is not None else own_frame(h, r)
    h.closed()
    h.take(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. re-upload under passes in flight
# ---------------------------------------------------------------------------------------------------------------------------------
def sc_reupload(h, kinds):
    w, hh, d = DIMS['r8']
    vol = h.volume('r8', h.noise('r8', 21) >> 2)      # low codes: MIP keeps the largest sample of every pass, and the new box must show
    rs = [h.renderer(k, vol) for k in kinds]
    for r in rs:
        h.warm(r)
    box = (3, 2, 0, w - 3, hh - 2, d)
    blocks = sources(h, h.noise('r8', 22), [box])
    h.gate()
    for r in rs:
        passes(h, r, 2)                       # on the side streams, reading the old texels
    h.lag()
    produce_and_upload(h, vol, blocks, None)  # the blit waits for them; its source sits behind the gate
    for r in rs:
        passes(h, r)                          # their side streams must see the new bricks, atlas and records
    outs = [own_frame(h, r) for r in rs]
    h.closed()
    for o in outs:
        h.take(o)


def sc_upload_unbound(h, kind):
    w, hh, d = DIMS['r8']
    first = h.volume('r8', h.noise('r8', 23))
    second = h.volume('r8')
    r = h.renderer(kind, first)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 24), boxes('box', w, hh, d))
    h.gate()
    passes(h, r, 2)
    h.lag()
    produce_and_upload(h, second, blocks, None)   # no renderer is bound to it
    h.do('setVolume', r.setVolume, second)
    passes(h, r)
    out = own_frame(h, r)
    h.closed()
    h.take(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. derived volumes
# ---------------------------------------------------------------------------------------------------------------------------------
def derive(h, op, v, earlier, second):
    """the derived volume(s) of `op`, the last one to be rendered; every one is kept until the run ends"""
    if op == 'reduce':
        return [h.do('reduce', v.reduce, 1)]
    if op == 'smooth1':
        return [h.do('smooth(1)', v.smooth, 1)]
    if op == 'rank1':
        return [h.do('rank(1)', v.rank, 'median', 1)]
    if op == 'combine_earlier':
        return [h.do('combine', v.combine, earlier, 'max')]
    if op == 'combine_device':
        return [h.do('combine', v.combine, second, 'absdiff')]
    if op == 'window':
        return [h.do('window', v.window, 64, 192)]
    if op == 'gradient':
        return [h.do('derive_gradient', v.derive_gradient)]
    if op == 'resample_nearest':
        return [h.do('resample(nearest)', v.resample, 31, 19, 26, 'nearest')]
    if op == 'chain':
        a = h.do('smooth(1)', v.smooth, 1)
        b = h.do('window', a.window, 32, 224)
        return [a, b, h.do('reduce', b.reduce, 1)]
    if op == 'smooth3':
        return [h.do('smooth(n)', v.smooth, 3)]
    if op == 'rank2':
        return [h.do('rank(n)', v.rank, 'dilate', 2)]
    if op == 'resample_filtered':
        return [h.do('resample(filtered)', v.resample, 31, 19, 26, 'filtered')]
    if op == 'components_keep':
        c = h.own(h.do('components', v.components, 128, 255))
        return [h.do('keep', c.keep, 1, None)]
    if op == 'distance_channel':
        f = h.own(h.do('distance', v.distance, 128, 255))
        return [h.do('channel', f.channel, 1)]
    if op == 'graph_prune':                   # the labellings read counts back; the pruning drains the stream before it frees its bitmap
        g = h.own(h.do('graph', v.graph, 224, 255))
        return [h.do('graph.prune', g.prune, 20, (10, 14, 17), True, 3)]
    raise ValueError(op)


def sc_derive(h, op):
    w, hh, d = DIMS['r8']
    other = h.volume('r8', h.noise('r8', 31))
    v = h.volume('r8')
    second = h.volume('r8') if op == 'combine_device' else None
    r = h.renderer('mip', other)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 32), boxes('slab', w, hh, d))
    blocks2 = sources(h, h.noise('r8', 33), boxes('box', w, hh, d)) if second is not None else None
    tgt = h.target(r)
    h.gate()
    passes(h, r, 1)                           # split passes on another volume: its side streams are busy when the volume is derived
    h.lag()
    produce_and_upload(h, v, blocks)
    if second is not None:
        produce_and_upload(h, second, blocks2)
    made = derive(h, op, v, other, second)
    for m in made:
        h.own(m)
    h.do('setVolume', r.setVolume, made[-1])
    h.do('set_render_target', r.set_render_target, tgt.data_ptr(), bytes_of(h, tgt))
    passes(h, r, 2)
    h.closed()
    h.take(tgt)


def sc_graph_emitters(h):
    """A graph built before the gate (vpt_volume_graph blocks).  Behind the gate its class pair volume, a copy of its branch labelling and
    that copy's label volume are only enqueued: vpt_graph_classes and the hand-out launch a kernel or a copy and return, and
    vpt_components_label of the copy does the same.  The first copy the consumer takes is the pair volume under passes, the second the
    label volume and then the volume the producer filled, accumulated (MIP keeps the maximum).  Only that last volume depends on the
    producer: it alone tells stale inputs from fresh ones.  The pair and the label volume come from texels uploaded before the gate, so
    the scenario shows that the three entries do not wait for the host and that their bytes are the twin's beside split passes and a
    producer's upload, not that they order behind producer work."""
    w, hh, d = DIMS['r8']
    kept = h.volume('r8', h.noise('r8', 34))
    g = h.own(kept.graph(224, 255))
    v = h.volume('r8')
    r = h.renderer('mip', kept)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 35), boxes('slab', w, hh, d))
    tgt = h.target(r)
    h.gate()
    passes(h, r, 1)
    h.lag()
    produce_and_upload(h, v, blocks)
    pair = h.own(h.do('graph.classes', g.classes))
    branches = h.own(h.do('graph.branch_components', getattr, g, 'branches'))
    label = h.own(h.do('label', branches.label))
    h.do('set_render_target', r.set_render_target, tgt.data_ptr(), bytes_of(h, tgt))
    h.do('setVolume', r.setVolume, pair)
    h.do('reset', r.reset)
    passes(h, r, 2)
    h.take(tgt)
    h.do('setVolume', r.setVolume, label)
    h.do('reset', r.reset)
    passes(h, r, 1)
    h.do('setVolume', r.setVolume, v)
    passes(h, r, 2)
    h.closed()
    h.take(tgt)
    h.check('the class pair and the label volume show in the frames', lambda outs: outs[0].any() and outs[1].any() and not (outs[0] == outs[1]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# D. tables changed between split passes
# ---------------------------------------------------------------------------------------------------------------------------------
def sc_tables(h, kind, change):
    np, N = h.env.np, h.env.N
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer(kind, vol)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 41), boxes('slab', w, hh, d))
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    passes(h, r, 2)
    h.take(own_frame(h, r))                   # the earlier frame keeps the old table
    h.lag()
    if change == 'tf':
        h.do('setTransferFunction', r.setTransferFunction, h.env.synthetic.colour_tf(48, 1))
    elif change == 'env':
        texels = np.random.default_rng(42).random((4, 8, 4), dtype=np.float32)
        texels[..., 3] = 1.0
        h.do('set_environment_texels', r.setEnvironmentMap, texels)
    elif change == 'filter':
        h.do('setFilter', vol.setFilter, 'nearest')
    elif change == 'options' and kind == 'mcm':
        h.do('set_option', r.set_option, N.OPTION_BOUNDARY_ATLAS, 0)
        h.do('set_option', r.set_option, N.OPTION_TILE_CLASSES, 0)
    elif change == 'options':
        h.do('set_option', r.set_option, N.OPTION_SPLIT_STREAMS, 2)
        h.do('set_option', r.set_option, N.OPTION_TILE_CLASSES, 0)
    if kind != 'mip':
        h.do('reset', r.reset)                # (the accumulating renderers start over, as the property handlers do)
    passes(h, r, 2)
    out = own_frame(h, r)
    h.closed()
    h.take(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# E. tone mapper
# ---------------------------------------------------------------------------------------------------------------------------------
def tonemapped(h, tm):
    h.do('tonemapper.render', tm.render)
    import ctypes as C
    N = h.env.N

    def output_device():
        p, n = C.c_void_p(), C.c_size_t(0)
        N.check(N.lib().vpt_tonemapper_output_device(tm._h, C.byref(p), C.byref(n)))
        return p.value, n.value
    ptr, nbytes = h.do('tonemapper.output_device', output_device)
    return h.view(ptr, nbytes)


def sc_tonemap(h, kind, table, fuse, resize):
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer(kind, vol, white=True)
    tm = h.tonemapper(r, table, fuse)
    h.warm(r)
    tm.render()                               # (table form with FUSE on: from here on r's fused passes write the RGBA8 image themselves)
    blocks = sources(h, h.noise('r8', 51), boxes('slab', w, hh, d))
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    passes(h, r, 2)
    out = tonemapped(h, tm)
    if not resize:
        h.closed()
    h.take(out)
    if resize:
        h.do('resize', r.setResolution, (176, 112))
        h.do('resize', tm.setResolution, (176, 112))
        passes(h, r, 2)
        h.take(tonemapped(h, tm))


# ---------------------------------------------------------------------------------------------------------------------------------
# F. buckets and frame sequences
# ---------------------------------------------------------------------------------------------------------------------------------
SLOTS = 4


def sc_play_into(h, kind, again):
    torch = h.env.torch
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer(kind, vol, white=again)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 61), boxes('slab', w, hh, d))
    bucket = h.zeros((SLOTS, H, W, 4), torch.float16)
    h.targets.append(r)
    stride = bytes_of(h, bucket[0])
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    h.do('play_into', r.play_into, SLOTS, bucket.data_ptr(), stride)
    if again:
        # The caller overwrites a slot from the stream and asks for the next bucket in the same memory.  The library requires
        # vpt_renderer_set_render_target on the memory the caller wrote (include/vpt.h): without it a later pass may skip texels it
        # knows it has written before.  That documented sequence is what runs here.
        h.take(bucket)
        h.lag()
        marker = 12344.0                      # a half no frame holds
        h.torch_op(bucket[1].fill_, marker)
        h.do('set_render_target', r.set_render_target, bucket[1].data_ptr(), stride)
        h.do('play_into', r.play_into, SLOTS, bucket.data_ptr(), stride)
        pattern = h.env.np.frombuffer(h.env.np.float16(marker).tobytes(), h.env.np.uint16)[0]
        h.check('no texel of the second bucket holds what the caller wrote into slot 1',
                lambda outs: not (outs[-1].view(h.env.np.uint16) == pattern).any())
    h.closed()
    h.take(bucket)


def sc_play_into_display(h, kind):
    torch = h.env.torch
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer(kind, vol)
    tm = h.tonemapper(r, True, True)
    h.warm(r)
    tm.render()                               # arms the tone mapper on r
    blocks = sources(h, h.noise('r8', 62), boxes('slab', w, hh, d))
    bucket = h.zeros((SLOTS, H, W, 4), torch.uint8)
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    h.do('play_into_display', r.play_into_display, tm, SLOTS, bucket.data_ptr(), bytes_of(h, bucket[0]))
    h.closed()
    h.take(bucket)


def sc_play_frames(h):
    import ctypes as C
    N = h.env.N
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer('mcm', vol)
    h.warm(r)
    r.play(2, frames=True)                    # (the frame ring is allocated on first use)
    blocks = sources(h, h.noise('r8', 63), boxes('slab', w, hh, d))
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    h.do('play(frames)', r.play, SLOTS, frames=True)

    def ring():
        p, n = C.c_void_p(), C.c_size_t(0)
        N.check(N.lib().vpt_renderer_frame_ring_device(r._h, C.byref(p), C.byref(n)))
        return p.value, n.value
    ptr, slot_bytes = h.do('frame_ring_device', ring)
    h.closed()
    h.take(h.view(ptr, slot_bytes * SLOTS))


def sc_play_fused(h, kind):
    w, hh, d = DIMS['r8']
    vol = h.volume('r8')
    r = h.renderer(kind, vol)
    h.warm(r)
    # The per-frame uniforms go through a device ring of 2048 entries.  One turn of it before the gate: an entry read too early then holds
    # this run's frame of 2048 frames ago, not whatever the memory held (a freed ring of the twin run holds the right values).
    for _ in range(4):
        r.play(512, fused=True)
    blocks = sources(h, h.noise('r8', 64), boxes('slab', w, hh, d))
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('reset', r.reset)
    # every stream reads the per-frame uniforms a call uploads on the context's stream.  (The second fused pass behind a reset builds the
    # marchers' tile lists, which joins and forks by itself: the third call is the one only the upload orders.)
    h.do('play(fused)', r.play, 2, fused=True)
    h.do('play(fused)', r.play, 2, fused=True)
    h.lag()
    h.do('play(fused)', r.play, 2, fused=True)
    out = own_frame(h, r)
    h.closed()
    h.take(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# G. lifetime on a caller's stream
# ---------------------------------------------------------------------------------------------------------------------------------
def sc_destroy_objects(h):
    w, hh, d = DIMS['r8']
    kept = h.volume('r8', h.noise('r8', 71))
    source = h.volume('r8')
    ra = h.renderer('mcs', kept)
    rb = h.renderer('mip', kept)
    doomed = h.renderer('eam', kept)
    tm = h.tonemapper(ra, True, True)
    tm_doomed = h.tonemapper(doomed, True, True)
    for r in (ra, rb, doomed):
        h.warm(r)
    tm.render(); tm_doomed.render()
    blocks = sources(h, h.noise('r8', 72), boxes('slab', w, hh, d))
    tgt = h.target(rb)
    h.gate()
    produce_and_upload(h, source, blocks)
    smoothed = h.own(h.do('smooth(1)', source.smooth, 1))
    passes(h, ra, 2)
    passes(h, doomed, 2)
    h.do('tonemapper.render', tm_doomed.render)
    h.do('destroy', source.destroy)           # work that reads it is queued behind the gate
    h.do('destroy', doomed.destroy)
    h.do('destroy', tm_doomed.destroy)
    h.do('setVolume', rb.setVolume, smoothed)
    h.do('set_render_target', rb.set_render_target, tgt.data_ptr(), bytes_of(h, tgt))
    passes(h, rb, 2)
    passes(h, ra, 1)
    h.take(tgt)
    h.take(own_frame(h, ra))
    h.take(tonemapped(h, tm))


def sc_destroy_context(h):
    torch, np = h.env.torch, h.env.np
    w, hh, d = DIMS['r8']
    mine = h.env.vpt.Context(0, stream=h.env.stream.cuda_stream)
    h.ctx = mine
    vol = h.volume('r8')
    r = h.renderer('mip', vol)
    h.warm(r)
    blocks = sources(h, h.noise('r8', 73), boxes('slab', w, hh, d))
    tgt = h.target(r)
    h.gate()
    produce_and_upload(h, vol, blocks)
    h.do('set_render_target', r.set_render_target, tgt.data_ptr(), bytes_of(h, tgt))
    h.do('reset', r.reset)
    passes(h, r, 2)
    h.take(tgt)
    h.do('destroy', r.destroy)
    h.do('destroy', vol.destroy)
    h.ctx = None
    h.do('context.destroy', mine.destroy)
    after = h.torch_op(lambda: torch.arange(4096, device=h.env.dev, dtype=torch.int32) * 3 + 1)   # the stream is the caller's: still usable
    h.take(after)
    h.check('a torch kernel on the stream behind vpt_context_destroy computes what it should',
            lambda outs: np.array_equal(outs[-1].view(np.int32), np.arange(4096, dtype=np.int32) * 3 + 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
def scenario(name, family, waits, fn, entries, **params):
    return {'name': name, 'family': family, 'waits': waits, 'fn': fn, 'entries': tuple(sorted(set(entries))), 'params': params}


def _table():
    t = []
    own = ['join', 'render_buffer_device']
    up = ['upload_block_device', 'finalize']
    # A
    for fmt, path in (('r8', 'slab'), ('r8', 'box'), ('r16', 'slab'), ('r16', 'box'), ('rgb565', 'box')):
        for kind in ('mip', 'mcm', 'mcs'):
            for target in ('own', 'caller'):
                packed = fmt == 'rgb565'       # decoded into float storage: its finalize scans for non-finite texels and waits
                t.append(scenario('A_%s_%s_%s_%s' % (fmt, path, kind, target), 'A', 'blocking' if packed else 'asynchronous', sc_upload,
                                  ['upload_block_device', 'finalize(float)' if packed else 'finalize', 'reset', 'render'] +
                                  (own if target == 'own' else ['set_render_target']), path=path, fmt=fmt, kind=kind, target=target))
    # B
    for name, kinds in (('mip', ('mip',)), ('mcm', ('mcm',)), ('mip_and_mcs', ('mip', 'mcs'))):
        t.append(scenario('B_reupload_%s' % name, 'B', 'asynchronous', sc_reupload, ['upload_block_device', 'render'] + own, kinds=kinds))
    for kind in ('mip', 'mcm'):
        t.append(scenario('B_upload_unbound_then_bind_%s' % kind, 'B', 'asynchronous', sc_upload_unbound,
                          ['upload_block_device', 'render', 'setVolume'] + own, kind=kind))
    # C
    derived = ['render', 'setVolume', 'set_render_target'] + up
    for op, entries in (('reduce', ['reduce']), ('smooth1', ['smooth(1)']), ('rank1', ['rank(1)']), ('combine_earlier', ['combine']),
                        ('combine_device', ['combine']), ('window', ['window']), ('gradient', ['derive_gradient']),
                        ('resample_nearest', ['resample(nearest)']), ('chain', ['smooth(1)', 'window', 'reduce'])):
        t.append(scenario('C_%s' % op, 'C', 'asynchronous', sc_derive, derived + entries, op=op))
    for op, entries in (('smooth3', ['smooth(n)']), ('rank2', ['rank(n)']), ('resample_filtered', ['resample(filtered)']),
                        ('components_keep', ['components', 'keep']), ('distance_channel', ['distance', 'channel']),
                        ('graph_prune', ['graph', 'graph.prune'])):
        t.append(scenario('C_%s' % op, 'C', 'blocking', sc_derive, derived + entries, op=op))
    t.append(scenario('C_graph_emitters', 'C', 'asynchronous', sc_graph_emitters,
                      derived + ['reset', 'graph.classes', 'graph.branch_components', 'label']))
    # D
    tables = up + ['reset', 'render'] + own
    for kind, change, waits, entries in (('mip', 'tf', 'blocking', ['setTransferFunction']), ('mcm', 'tf', 'blocking', ['setTransferFunction']),
                                         ('mcs', 'env', 'blocking', ['set_environment_texels']), ('mcm', 'env', 'blocking', ['set_environment_texels']),
                                         ('mip', 'filter', 'asynchronous', ['setFilter']), ('mcm', 'filter', 'asynchronous', ['setFilter']),
                                         ('mip', 'options', 'asynchronous', ['set_option']), ('mcm', 'options', 'asynchronous', ['set_option'])):
        t.append(scenario('D_%s_%s' % (change, kind), 'D', waits, sc_tables, tables + entries, kind=kind, change=change))
    # E
    tone = up + ['reset', 'render', 'tonemapper.render', 'tonemapper.output_device']
    for name, kind, table, fuse in (('fused_table_mip', 'mip', True, True), ('fused_table_mcm', 'mcm', True, True),
                                    ('separate_table_mip', 'mip', True, False), ('direct_mip', 'mip', False, True)):
        t.append(scenario('E_%s' % name, 'E', 'asynchronous', sc_tonemap, tone, kind=kind, table=table, fuse=fuse, resize=False))
    for name, kind, table, fuse in (('fused_table_mip', 'mip', True, True), ('direct_mip', 'mip', False, True)):
        t.append(scenario('E_%s_resized' % name, 'E', 'blocking', sc_tonemap, tone + ['resize'], kind=kind, table=table, fuse=fuse, resize=True))
    # F
    for kind in ('mip', 'depth', 'mcm'):
        t.append(scenario('F_play_into_%s' % kind, 'F', 'asynchronous', sc_play_into, up + ['reset', 'play_into'], kind=kind, again=False))
    for kind in ('mip', 'mcm'):
        t.append(scenario('F_play_into_again_%s' % kind, 'F', 'asynchronous', sc_play_into,
                          up + ['reset', 'play_into', 'set_render_target'], kind=kind, again=True))
    for kind in ('eam', 'mcm'):
        t.append(scenario('F_play_into_display_%s' % kind, 'F', 'asynchronous', sc_play_into_display, up + ['reset', 'play_into_display'], kind=kind))
    t.append(scenario('F_play_frames_mcm', 'F', 'asynchronous', sc_play_frames, up + ['reset', 'play(frames)', 'frame_ring_device']))
    for kind in ('mip', 'eam'):
        t.append(scenario('F_play_fused_%s' % kind, 'F', 'asynchronous', sc_play_fused, up + ['reset', 'play(fused)'] + own, kind=kind))
    # G
    t.append(scenario('G_destroy_volume_renderer_tonemapper', 'G', 'blocking', sc_destroy_objects,
                      up + ['smooth(1)', 'render', 'tonemapper.render', 'tonemapper.output_device', 'destroy', 'setVolume',
                            'set_render_target'] + own))
    t.append(scenario('G_destroy_context', 'G', 'blocking', sc_destroy_context,
                      up + ['set_render_target', 'reset', 'render', 'destroy', 'context.destroy']))
    return t


SCENARIOS = _table()


# ---------------------------------------------------------------------------------------------------------------------------------
# running
# ---------------------------------------------------------------------------------------------------------------------------------
def run_once(env, sc, mode):
    h = Harness(env, mode)
    with env.torch.cuda.stream(env.stream):
        sc['fn'](h, **sc['params'])
        outs = h.finish()
    return h, outs


def judge(env, sc):
    """(passed, report) of one scenario: its runs and what is asserted about them"""
    np = env.np
    twin_h, twin = run_once(env, sc, 'twin')
    _, stale = run_once(env, sc, 'stale')
    t0 = time.perf_counter()
    h, got = run_once(env, sc, 'ordered')
    rep = {'waits': sc['waits'], 'ordered_run_ms': round((time.perf_counter() - t0) * 1e3, 1)}
    problems = []
    # the bytes
    first = None
    if len(got) != len(twin):
        first = 'the ordered run took %d copies, the twin run %d' % (len(got), len(twin))
    for k, (a, b) in enumerate(zip(got, twin)):
        if first is None and (a.shape != b.shape or not np.array_equal(a, b)):
            if a.shape != b.shape:
                first = 'copy %d: %d bytes against %d' % (k, a.size, b.size)
            else:
                d = np.flatnonzero(a != b)
                first = 'copy %d, byte %d: %d against the twin\'s %d (%d of %d bytes differ)' % (k, d[0], a[d[0]], b[d[0]], d.size, a.size)
    rep['first_difference'] = first
    if first is not None:
        problems.append('ordered run differs from the synchronised twin: ' + first)
    # the stale twin
    total = sum(a.size for a in twin)
    differ = sum(int(np.count_nonzero(a != b)) if a.shape == b.shape else a.size for a, b in zip(stale, twin))
    rep['stale_fraction'] = round(differ / max(total, 1), 4)
    if rep['stale_fraction'] < STALE_FRACTION:
        problems.append('the stale twin differs in %.2f %% of the bytes only: the scenario cannot tell stale inputs' % (100 * rep['stale_fraction']))
    # the gate
    rep['gate'] = None if h.gate_pending is None else ('closed' if h.gate_pending else 'open')
    rep['enqueue_ms'] = None if h.enqueue_ms is None else round(h.enqueue_ms, 3)
    rep['gate_ms'] = None if h.gate_ms is None else round(h.gate_ms, 2)
    if sc['waits'] == 'asynchronous' and rep['gate'] != 'closed':
        slow = max(h.calls, key=lambda c: c[1]) if h.calls else ('-', 0.0)
        problems.append('the gate was %s when the last library call returned (slowest call: %s, %.2f ms)' %
                        (rep['gate'] or 'never looked at', slow[0], slow[1]))
    # the entries
    for which, hh in (('twin', twin_h), ('ordered', h)):
        if hh.used != set(sc['entries']):
            problems.append('%s run called %s, the table lists %s' % (which, sorted(hh.used), sorted(sc['entries'])))
            break
    # the scenario's own properties
    for which, hh, outs in (('twin', twin_h, twin), ('ordered', h, got)):
        for what, fn in hh.checks:
            if not fn(outs):
                problems.append('%s run: not so: %s' % (which, what))
    rep['problems'] = problems
    return not problems, rep


def calibrate(env):
    """milliseconds per cycle of torch.cuda._sleep on this device"""
    torch = env.torch
    out = {}
    with torch.cuda.stream(env.stream):
        for cycles in (1000000, 10000000):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            e0.record(); torch.cuda._sleep(cycles); e1.record()
            queued = not e1.query()
            torch.cuda.synchronize()
            out[cycles] = (e0.elapsed_time(e1), queued)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='run the scenarios whose name contains this')
    ap.add_argument('--gate-cycles', type=int, default=GATE_CYCLES)
    ap.add_argument('--gate-ms', type=float, default=None, help='(for measurements) size the gate from a calibration run instead')
    args = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import vpt_amd
    from vpt_amd import _native, scene, synthetic

    env = Env()
    env.np, env.torch, env.vpt, env.N, env.scene, env.synthetic = np, torch, vpt_amd, _native, scene, synthetic
    env.dev = torch.device('cuda:0')
    torch.cuda.set_device(env.dev)
    env.stream = torch.cuda.Stream(device=env.dev)
    env.gate_cycles = args.gate_cycles
    t_start = time.perf_counter()
    if args.gate_ms is not None:
        cal = calibrate(env)
        per_cycle = cal[10000000][0] / 1e7
        env.gate_cycles = int(args.gate_ms / per_cycle)
        print('CALIBRATION\t%s' % json.dumps({'ms': {str(k): round(v[0], 3) for k, v in cal.items()}, 'ms_per_cycle': per_cycle,
                                               'still_queued_on_return': [v[1] for v in cal.values()], 'gate_cycles': env.gate_cycles}))
    with torch.cuda.stream(env.stream):
        env.ctx = vpt_amd.Context(0, stream=env.stream.cuda_stream)
    failed = 0
    for sc in SCENARIOS:
        if args.only and args.only not in sc['name']:
            continue
        try:
            ok, rep = judge(env, sc)
        except Exception as e:                # a HIP error, or anything else that leaves the device in an unknown state: stop here
            import traceback
            print('RESULT\t%s\tERROR\t%s' % (sc['name'], json.dumps({'problems': ['%s: %s' % (type(e).__name__, e)],
                                                                       'traceback': traceback.format_exc()[-1500:]})))
            sys.stdout.flush()
            return 3
        failed += 0 if ok else 1
        print('RESULT\t%s\t%s\t%s' % (sc['name'], 'PASS' if ok else 'FAIL', json.dumps(rep)))
        sys.stdout.flush()
    env.ctx.destroy()
    print('WORKER\t%s' % json.dumps({'seconds': round(time.perf_counter() - t_start, 2), 'gate_cycles': env.gate_cycles, 'failed': failed}))
    sys.stdout.flush()
    return 1 if failed else 0


if __name__ == '__main__':
    sys.exit(main())
