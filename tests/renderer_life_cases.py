"""Fixed-seed renderer LIVES: what happens to one renderer object between its construction and its destruction, drawn from numpy's
generator alone (no device: the only native call is the host-only vpt_classify_tiles).  The cases of tests/test_gpu_renderer_life.py,
which replays every life on the device beside the CPU oracle; tests/test_renderer_life_cases.py holds the drawn set to the conditions
without which that test would check little.

Kinds: mip, eam, mcs, mcm, iso, depth, lao.  DOS is swept slice by slice by its own driver, tests/test_gpu_dos.py, and has no frame
sequences, shards, split streams or tile classes: it stays there.

``setup(kind, seed)`` is everything a replay needs; ``life(kind, seed)`` its event list; ``describe(kind, seed)`` the same as a
Python-like script, which goes into every assertion message.  An event is a dict of plain numbers, strings and small arrays:

  render n | play n mode (graph, eager, fused, frames) | play_into n bucket | play_into_display n          the passes
  reset | camera cam reset | transform model | lens fovy near far                                          resets and matrix changes
  fused value | tf tf via (direct: no reset; property: the handler resets) | env env | prop name value     uniforms and tables
  filter vol name | upload vol at block | wide vol value | set_volume vol (resets)                          the volume
  resize size (resets) | option option value | target to (0, 1: a holder's render buffer; None: the own buffer)
  tm_create kind | tm_render | tm_params values | tm_option option value | tm_destroy                      the tone mapper
  read buffers twice | sample_count                                                                         reads in the middle

How a life is drawn.  Image 33..112 x 17..96, volumes of 2..24 voxels per axis (never cubic), one life in three a row shard.  Two lives
in three ask for a camera that sees the volume in some 16x16 tiles and misses it in others (drawn again, up to 24 times, until the
host's classification says so); the rest sit inside the volume or fill the image with it.  A life follows SLOTS: pass events (the
first one two or more render() calls, the others walking pass_entries) with the seed's five wishes between them — entries(kind) taken by
turns, five per seed, so that 24 seeds reach every entry three times; a wish that needs a tone mapper or a redirected target gets one
first — 9..12 events, at most 24 passes (LAO, whose pass is the dearest by far: 12).  Independent draws put too few perturbations
where they are worth most, between two runs of fused passes under one reset that saw both tile classes (armed()), so the lives that can
get there (two in three) sort their wishes — the resetting ones first, matrix changes last — and end with one more perturbation, taken by
turns from late_perturbations(kind), before their last passes.  A life's first properties leave out extinction 0 and isovalue 0 / 1,
at which no perturbation shows; those values come with the property events."""
import ctypes as C
import functools
import math
import types

import numpy as np

from vpt_amd import _native as N
from vpt_amd.scene import Node, Transform, PerspectiveCamera, quat, mvp_inverse_matrix

_real_lib = N.lib
CONSTANT = 0x4C494645
DEFAULT_SEEDS = (0, 24)
KINDS = ["mip", "eam", "mcs", "mcm", "iso", "depth", "lao"]
MAX_PASSES = 24
FORMATS = ('R8', 'RG8', 'R32F', 'R8_SNORM', 'R16', 'R16_SNORM', 'RG32F')
DTYPES = {'R8': np.uint8, 'RG8': np.uint8, 'R32F': np.float32, 'R8_SNORM': np.int8, 'R16': np.uint16, 'R16_SNORM': np.int16, 'RG32F': np.float32}
FILTERS = ('nearest', 'linear', 'quasicubic')
TF_WIDTHS = (1, 2, 7, 64, 256, 1024)
TONEMAPPERS = ("artistic", "range", "reinhard", "reinhard2", "uncharted2", "filmic", "unreal", "aces", "lottes", "uchimura")
ENV_FORMS = ('byte', 'alpha', 'byte2x3', 'float', 'half3x2')
# the properties whose 'change' handler resets (the reference's handlers, as vpt_amd/renderers.py cites them)
RESET_ON = {'mip': ('transferFunction',), 'eam': ('extinction', 'slices', 'random', 'transferFunction'),
            'mcs': ('extinction', 'transferFunction'), 'mcm': ('extinction', 'anisotropy', 'bounces', 'transferFunction'),
            'iso': ('isovalue', 'transferFunction'), 'depth': ('extinction', 'slices', 'threshold', 'random', 'transferFunction'),
            'lao': ('extinction', 'slices', 'transferFunction')}
# property -> the values a life draws from (tests/test_gpu_fuzz.py run_random_scene's lists)
PROPERTIES = {
    'mip': {'steps': [1, 2, 3, 17, 64, 100]},
    'eam': {'slices': [1, 5, 33, 64], 'extinction': [0.0, 1.0, 40.0, 300.0], 'random': [False, True]},
    'mcs': {'extinction': [0.0, 0.5, 5.0, 60.0]},
    'mcm': {'extinction': [0.0, 1.0, 7.0, 80.0], 'anisotropy': [0.0, 0.9, -0.7, 1e-6], 'bounces': [0, 1, 8], 'steps': [1, 3, 8]},
    'iso': {'steps': [1, 2, 7, 50], 'isovalue': [0.0, 0.2, 0.5, 1.0], 'light': None},
    'depth': {'slices': [1, 9, 64], 'extinction': [0.0, 10.0, 100.0], 'threshold': [0.0, 0.1, 0.9], 'random': [False, True]},
    'lao': {'slices': [1, 7, 24], 'extinction': [0.0, 30.0, 100.0, 400.0], 'localAmbientOcclusion': [False, True], 'softShadows': [False, True],
            'LAOWeight': None, 'shadowsWeight': None, 'numLAOSamples': [1, 2, 3], 'numShadowSamples': [1, 4, 11],
            'LAOStepSize': [0.01, 0.05, 0.3, 1.5], 'lightRadious': [0.0, 0.19, 0.7], 'lightCoeficient': [0.5, 1.0, 3.0], 'lightPosition': None},
}
OPTIONS = {'split': (N.OPTION_SPLIT_STREAMS, (1, 2, 3)), 'classes': (N.OPTION_TILE_CLASSES, (0, 1, 2)), 'settled': (N.OPTION_SETTLED_MISS, (0, 1)),
           'atlas': (N.OPTION_BOUNDARY_ATLAS, (0, 1)), 'records': (N.OPTION_COLUMN_RECORDS, (0, 1)),
           'mcm_persistent': (N.OPTION_MCM_PERSISTENT, (0, 1, 2)), 'mcs_persistent': (N.OPTION_MCS_PERSISTENT, (0, 1)),
           'verify': (N.OPTION_VERIFY_TILE_CLASSES, (0, 1))}
OPTIONS_OF = {'mcm': ('split', 'classes', 'settled', 'atlas', 'records', 'mcm_persistent', 'verify'), 'mcs': ('split', 'classes', 'mcs_persistent'),
              'lao': ('split',)}
ENV_KINDS = ('mcs', 'mcm')                             # the renderers whose shaders read the environment map
PASS_OPS = ('render', 'play', 'play_into', 'play_into_display')
# the events that change what later passes compute or how they are launched, without a reset of their own
PERTURBING = {'tf': 'tf', 'env': 'env', 'camera': 'matrix', 'transform': 'matrix', 'lens': 'matrix', 'filter': 'filter', 'upload': 'upload_block',
              'option': 'option', 'target': 'target', 'tm_create': 'tone mapper', 'tm_params': 'tone mapper', 'tm_option': 'tone mapper',
              'tm_destroy': 'tone mapper', 'fused': 'fused toggle'}
VISIBLE = ('tf', 'env', 'filter', 'upload', 'set_volume', 'prop')      # a twin without one of these must show another image


def options_of(kind):
    return OPTIONS_OF.get(kind, ('split', 'classes'))


def entries(kind):
    """the other-than-pass events a life of `kind` can hold, by the names the wishes and the coverage count use"""
    out = ['reset', 'camera_reset', 'camera', 'transform', 'lens', 'fused', 'tf_direct', 'tf_property', 'prop', 'filter', 'upload', 'wide',
           'set_volume', 'resize', 'target', 'target_none', 'tm_create', 'tm_render', 'tm_params', 'tm_fuse', 'tm_table', 'tm_destroy',
           'read', 'read_twice', 'sample_count']
    if kind in ENV_KINDS:
        out += ['env_' + f for f in ENV_FORMS]
    # (four entries twice: the wishes walk this list, and these are worth most in the armed position; MCM's list is long enough as it is)
    out += ['option_' + o for o in options_of(kind)] + (['fused', 'upload', 'tf_direct', 'filter'] if kind != 'mcm' else [])
    # ... in an order that keeps the entries of one family apart: a life's wishes are neighbours in this list, and a transfer function set
    # right after another one would hide the first
    stride = next(k for k in (11, 13, 17, 7) if math.gcd(k, len(out)) == 1)
    return [out[(i * stride) % len(out)] for i in range(len(out))]


def pass_entries(kind):
    out = ['render', 'play_graph', 'play_eager', 'play_into', 'play_into_display']
    if kind != 'lao':
        out.append('play_fused')
    if kind == 'mcm':
        out += ['play_frames', 'play_into_bucket']
    return out


def entry_of(e):
    """the entry an event counts for"""
    op = e['op']
    if op == 'play':
        return 'play_' + e['mode']
    if op == 'play_into':
        return 'play_into_bucket' if e['bucket'] else 'play_into'
    if op == 'camera':
        return 'camera_reset' if e['reset'] else 'camera'
    if op == 'tf':
        return 'tf_' + e['via']
    if op == 'env':
        return 'env_' + e['form']
    if op == 'option':
        return 'option_' + e['option']
    if op == 'target':
        return 'target_none' if e['to'] is None else 'target'
    if op == 'tm_option':
        return 'tm_' + e['option']
    if op == 'read':
        return 'read_twice' if e['twice'] else 'read'
    return op


# ---- scene pieces ------------------------------------------------------------------------------------------------------------
def build_camera(cam, aspect):
    """the camera node of a drawn camera (yaw, pitch, dist, off, turn; fovy, near, far): tests/test_gpu_fuzz.py random_camera's construction"""
    node = Node()
    q = quat.multiply(quat.create(), quat.setAxisAngle(quat.create(), [0, 1, 0], cam['yaw']), quat.setAxisAngle(quat.create(), [1, 0, 0], cam['pitch']))
    if cam['turn']:
        q = quat.multiply(quat.create(), q, quat.setAxisAngle(quat.create(), [0, 1, 0], cam['turn']))
    node.transform.localRotation = q
    move_camera(node, cam)
    pc = PerspectiveCamera(node, {'fovy': cam['fovy'], 'aspect': aspect, 'near': cam['near'], 'far': cam['far']})
    node.components.append(pc)
    return node


def move_camera(node, cam):
    q = quat.multiply(quat.create(), quat.setAxisAngle(quat.create(), [0, 1, 0], cam['yaw']), quat.setAxisAngle(quat.create(), [1, 0, 0], cam['pitch']))
    if cam['turn']:
        q = quat.multiply(quat.create(), q, quat.setAxisAngle(quat.create(), [0, 1, 0], cam['turn']))
    node.transform.localRotation = q
    cy, sy, cp, sp = math.cos(cam['yaw']), math.sin(cam['yaw']), math.cos(cam['pitch']), math.sin(cam['pitch'])
    d, off = cam['dist'], cam['off']
    node.transform.localTranslation = [d * sy * cp + off[0], -d * sp + off[1], d * cy * cp + off[2]]


def set_lens(node, lens):
    pc = node.getComponent(PerspectiveCamera)
    pc.fovy, pc.near, pc.far = lens['fovy'], lens['near'], lens['far']


def set_model(transform, model):
    transform.localScale = list(model['scale'])
    transform.localTranslation = list(model['translation'])
    transform.localRotation = quat.setAxisAngle(quat.create(), [0.3, 0.8, 0.52], model['angle'])


def decode(texels, fmt):
    """the texels as the oracle takes them: bytes as they are, floats as they are, the normalised formats as the R32F values they read as"""
    t = np.asarray(texels)
    if fmt in ('R8', 'RG8', 'R32F', 'RG32F'):
        return t
    if fmt == 'R8_SNORM':
        return np.maximum(t.astype(np.float64) / 127.0, -1.0).astype(np.float32)
    if fmt == 'R16':
        return (t.astype(np.float64) / 65535.0).astype(np.float32)
    if fmt == 'R16_SNORM':
        return np.maximum(t.astype(np.float64) / 32767.0, -1.0).astype(np.float32)
    raise ValueError(fmt)


def channels(fmt):
    return 2 if fmt in ('RG8', 'RG32F') else 1


def _texels(rng, fmt, dims, special):
    """a noisy blob in the format's own codes over its whole range; R32F / RG32F reach outside [0, 1]"""
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) for n in dims], indexing='ij')
    u = np.clip(1.0 - np.sqrt(x * x + y * y + z * z) / 1.2 + rng.normal(0, 0.12, size=dims), 0.0, 1.0)
    if rng.uniform() < 0.25:
        u = rng.uniform(0, 1, size=dims)

    def code(u):
        if fmt in ('R8', 'RG8'):
            return np.rint(u * 255).astype(np.uint8)
        if fmt == 'R8_SNORM':
            return np.rint(u * 255 - 128).astype(np.int8)
        if fmt == 'R16':
            return np.rint(u * 65535).astype(np.uint16)
        if fmt == 'R16_SNORM':
            return np.rint(u * 65535 - 32768).astype(np.int16)
        return (u * 1.7 - 0.35).astype(np.float32)
    t = code(u)
    if channels(fmt) == 2:
        t = np.ascontiguousarray(np.stack([t, code(rng.uniform(0, 1, size=dims))], axis=-1))
    if special:                                           # one NaN and one Inf texel
        flat = t.reshape(-1)
        flat[int(rng.integers(0, flat.size))] = np.nan
        flat[int(rng.integers(0, flat.size))] = np.inf
    return t


def _dims(rng):
    while True:
        d = tuple(int(v) for v in rng.integers(2, 25, size=3))
        if len(set(d)) > 1:
            return d


def _camera(rng, mode):
    """mode 0: orbiting at a distance, the volume in the middle of the image (HIT and MISS tiles); 1: inside; 2: filling the image"""
    if mode == 0:
        cam = dict(yaw=float(rng.uniform(-math.pi, math.pi)), pitch=float(rng.uniform(-1.0, 1.0)), dist=float(rng.uniform(2.2, 5.0)),
                   off=[float(v) for v in rng.uniform(-0.25, 0.25, size=3)], turn=0.0, fovy=float(rng.uniform(0.6, 1.3)))
    elif mode == 1:
        cam = dict(yaw=float(rng.uniform(-math.pi, math.pi)), pitch=float(rng.uniform(-1.2, 1.2)), dist=float(rng.uniform(0.0, 0.4)),
                   off=[0.0, 0.0, 0.0], turn=0.0, fovy=float(rng.uniform(0.5, 1.5)))
    else:
        cam = dict(yaw=float(rng.uniform(-0.3, 0.3)), pitch=float(rng.uniform(-0.3, 0.3)), dist=float(rng.uniform(0.7, 1.0)),
                   off=[0.0, 0.0, 0.0], turn=0.0, fovy=float(rng.uniform(1.2, 1.6)))
    cam['near'] = float(rng.choice([0.01, 0.1, 0.5])); cam['far'] = float(rng.choice([10.0, 100.0]))
    return cam


def _model(rng):
    if rng.uniform() < 0.5:
        return dict(scale=[1.0, 1.0, 1.0], translation=[0.0, 0.0, 0.0], angle=0.0)
    return dict(scale=[float(v) for v in rng.uniform(0.6, 1.5, size=3)], translation=[float(v) for v in rng.uniform(-0.15, 0.15, size=3)],
                angle=float(rng.uniform(-1, 1)))


def _tf(rng, two_channels):
    w = int(rng.choice(TF_WIDTHS))
    h = 3 if two_channels and rng.uniform() < 0.5 else 1
    return rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def _env(rng, form):
    if form == 'byte':
        e = rng.integers(0, 256, size=(1, 1, 4), dtype=np.uint8); e[..., 3] = 255
    elif form == 'alpha':
        e = rng.integers(0, 256, size=(1, 1, 4), dtype=np.uint8); e[..., 3] = int(rng.integers(0, 255))
    elif form == 'byte2x3':
        e = rng.integers(0, 256, size=(3, 2, 4), dtype=np.uint8)
    elif form == 'float':                                 # a colour the running mean 1 + (e - 1) does not return to: e has to be kept, not recomputed
        while True:
            c = rng.uniform(0.05, 1.9, size=3).astype(np.float32)
            if all(np.float32(1) + (v - np.float32(1)) != v for v in c):
                break
        e = np.array([[[c[0], c[1], c[2], 1.0]]], dtype=np.float32)
    else:
        e = rng.uniform(0, 2.5, size=(2, 3, 4)).astype(np.float16); e[..., 3] = 1.0
    return e


def _size(rng):
    return int(rng.integers(33, 113)), int(rng.integers(17, 97))


def matrix_of(cam, model, aspect):
    node = build_camera(cam, aspect)
    tr = Transform(Node())
    set_model(tr, model)
    return mvp_inverse_matrix(node, tr)


def classify(w, h, m, shard):
    """(HIT tiles, MISS tiles) of the host-only vpt_classify_tiles for the shard's local rows"""
    rank, world, rows = shard or (0, 1, 1)
    L = _real_lib()                                       # (not N.lib(): inside test_gpu_fuzz.oracle_only() that is a stand-in that classifies nothing)
    tx, ty = C.c_int(0), C.c_int(0)
    m = np.ascontiguousarray(m, dtype=np.float32)
    N.check(L.vpt_classify_tiles(w, h, rank, world, rows, m.ctypes.data_as(C.c_void_p), None, 0, C.byref(tx), C.byref(ty)))
    cls = np.zeros(tx.value * ty.value, dtype=np.uint8)
    N.check(L.vpt_classify_tiles(w, h, rank, world, rows, m.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), cls.size, C.byref(tx), C.byref(ty)))
    return int((cls == 0).sum()), int((cls != 0).sum())


def _mixed_camera(rng, size, model, shard, aspect):
    cam = None
    for _ in range(24):
        cam = _camera(rng, 0)
        hit, miss = classify(size[0], size[1], matrix_of(cam, model, aspect), shard)
        if hit and miss:
            break
    return cam


# ---- the draw ------------------------------------------------------------------------------------------------------------------
def resets_of(kind, e):
    """how many times the event resets the renderer"""
    op = e['op']
    if op in ('reset', 'set_volume', 'resize'):
        return 1
    if op == 'camera':
        return 1 if e['reset'] else 0
    if op == 'tf':
        return 1 if e['via'] == 'property' else 0
    if op == 'prop':
        return 1 if e['name'] in RESET_ON[kind] else 0
    return 0


def passes_of(e):
    return e['n'] if e['op'] in PASS_OPS else 0


@functools.lru_cache(maxsize=None)
def setup(kind, seed):
    """one drawn life: kind, seed, size, shard, aspect, cam, model, volumes [(format, filter, texels)], tf, env, props, fast, lazy, early
    (what is destroyed before the renderer: None, 'volume', 'tonemapper'), events, and resets: for every reset of the life, the first included,
    (event index or -1, size, matrix, bound volume, its filter)"""
    rng = np.random.default_rng([CONSTANT, KINDS.index(kind), seed])
    s = types.SimpleNamespace(kind=kind, seed=seed)
    s.size = _size(rng)
    s.aspect = s.size[0] / s.size[1]
    s.shard = (lambda world: (int(rng.integers(0, world)), world, int(rng.choice([1, 3, 8, 16]))))(int(rng.integers(2, 4))) if seed % 3 == 1 else None
    s.model = _model(rng)
    mode = 0 if seed % 3 != 2 else int(rng.integers(1, 3))
    s.cam = _mixed_camera(rng, s.size, s.model, s.shard, s.aspect) if mode == 0 else _camera(rng, mode)
    # three volumes: the first bound at construction (every second life R8, what most options are written for), the others for setVolume
    first = 'R8' if seed % 2 == 0 else FORMATS[1 + (seed // 2) % (len(FORMATS) - 1)]
    fmts = [first, FORMATS[(seed + 1) % len(FORMATS)], FORMATS[(seed + 4) % len(FORMATS)]]
    s.volumes = []
    for k, fmt in enumerate(fmts):
        special = fmt == 'R32F' and (seed + k) % 8 == 3
        filt = 'linear' if k == 0 and seed % 2 == 0 else str(rng.choice(FILTERS))
        s.volumes.append((fmt, filt, _texels(rng, fmt, _dims(rng), special)))
    s.tf = _tf(rng, channels(first) == 2) if rng.uniform() < 0.7 else None
    s.env = _env(rng, str(rng.choice(ENV_FORMS))) if kind in ENV_KINDS and rng.uniform() < 0.4 else None
    while True:
        s.props = {name: _value(rng, kind, name) for name in PROPERTIES[kind]}
        if _props_ok(s.props, True):
            break
    s.fast = kind == 'mcm' and seed % 4 == 3
    s.lazy = seed % 4 in (1, 2)                           # (half of the R8 lives too: a state read in the middle is MCM's catch-up)
    s.early = ('volume', 'tonemapper')[(seed // 4) % 2] if seed % 4 == 1 else None
    if kind == 'mcm' and seed < DEFAULT_SEEDS[1] and seed % 4 == 2 and seed % 3 != 2:
        s.env = None                                      # (the lives of _events' `owing`: the white environment settles at the reset)
    s.split = (None, 3, 2, None)[seed % 4]               # VPT_OPTION_SPLIT_STREAMS from the start (None: the library's default, one stream at these sizes)
    s.start = int(rng.integers(1, 50))                   # where the renderer's GoldenRatioRng starts
    _events(rng, s)
    return s


def _props_ok(p, first):
    """LAO: its dearest settings not all at once (the oracle's side of a life stays under 3 s); a life's FIRST properties: an extinction
    and an isovalue at which the volume shows (0 and 1 come with the property events), so that most perturbations change the image"""
    if 'LAOStepSize' in p and p['slices'] == 24 and (p['LAOStepSize'] == 0.01 or p['numShadowSamples'] == 11):
        return False
    return not first or (p.get('extinction', 1.0) != 0.0 and p.get('isovalue', 0.5) not in (0.0, 1.0) and p.get('threshold', 0.1) != 0.0)


def _value(rng, kind, name):
    vals = PROPERTIES[kind][name]
    if vals is not None:
        v = vals[int(rng.integers(0, len(vals)))]
        return v
    if name == 'light':
        return [float(v) for v in rng.uniform(-3, 3, size=3)]
    if name == 'lightPosition':
        return [float(v) for v in rng.uniform(-12, 12, size=3)]
    return float(rng.uniform(0, 1))


_RESETTING = ('reset', 'camera_reset', 'tf_property', 'prop', 'set_volume', 'resize')      # the wishes that reset (prop: most of the time)
SLOTS = "POOPOOPOAP"                                   # the slots of a life: 4 pass events, 5 wishes, one perturbation near the end (A)


def late_perturbations(kind):
    """what slot A takes by turns: one event of every perturbing sort, where a life has the most passes behind it and two more to come"""
    return ['tf_direct', 'filter', 'upload', 'fused', 'target', 'tm_params', 'option_split', 'camera'] + \
        (['env_byte', 'env_float'] if kind in ENV_KINDS else []) + (['option_classes'] if kind != 'lao' else [])


def _events(rng, s):
    kind, seed = s.kind, s.seed
    ent, pent, late = entries(kind), pass_entries(kind), late_perturbations(kind)
    st = types.SimpleNamespace(size=s.size, cam=dict(s.cam), model=dict(s.model), bound=0, filters=[v[1] for v in s.volumes], fused=True,
                               target=None, tm=None, tm_sat=1.0, budget=MAX_PASSES // 2 if kind == 'lao' else MAX_PASSES, props=dict(s.props),     # (LAO: the costliest pass by far)
                               options={o: None for o in OPTIONS})
    events = []
    s.resets = [(-1, st.size, matrix_of(st.cam, st.model, s.aspect), 0, st.filters[0])]
    others = passes = done = 0
    by_turns = seed < DEFAULT_SEEDS[1]                     # the default seeds meet the coverage conditions by turns; later seeds draw everything
    if by_turns:
        wishes = [ent[(seed * 5 + k) % len(ent)] for k in range(SLOTS.count('O'))]
        if seed % 3 != 2:                                  # (the lives whose first camera sees both tile classes)
            wishes.sort(key=lambda n: 0 if n in _RESETTING else 2 if n in ('camera', 'transform', 'lens') else 1)
        slots = SLOTS if seed % 3 != 2 else SLOTS.replace('A', '')    # (slot A is for the lives that can be in the armed position)
    else:
        wishes = [ent[int(rng.integers(0, len(ent)))] for _ in range(10)]
        slots = "P" + "".join(str(rng.choice(["O", "O", "P", "A"])) for _ in range(int(rng.integers(5, 10)))) + "P"
    # MCM, four default lives: a float / half environment map while the settled MISS kernel's samples are still owed (owed(): R8 volume, lazy
    # state checks, a white environment, two or more render() calls right before the map and nothing that would make the library catch up)
    owing = kind == 'mcm' and by_turns and seed % 4 == 2 and seed % 3 != 2
    if owing:
        slots = "PAPOOPOOOP"
    for at, slot in enumerate(slots):
        if len(events) >= 12:
            break
        after_perturbation = bool(events) and events[-1]['op'] in PERTURBING
        room = 12 - len(events) - (len(slots) - done - 1)  # events this slot may add and still leave one for every later slot
        done += 1
        if slot == 'P':
            if st.budget - (slots.count('P') - passes - 1) < 1:
                continue
            name = 'render' if passes == 0 or (owing and slots[at + 1:at + 2] == 'A') else \
                pent[(seed * 3 + passes - 1) % len(pent)] if by_turns else pent[int(rng.integers(0, len(pent)))]
            new = _pass_event(rng, s, st, name, after_perturbation or passes == 0 or owing, room, slots.count('P') - passes - 1)
            passes += 1
        elif slot == 'A':
            name = late[(seed - seed // 3) % len(late)] if by_turns else late[int(rng.integers(0, len(late)))]
            if owing:
                name = ('env_float', 'env_half3x2')[(seed // 4) % 2]
            new = _other_event(rng, s, st, name, room)
        elif room < 1:
            continue
        else:
            new = _other_event(rng, s, st, wishes[others], room)
            others += 1
        for e in new:
            events.append(e)
            st.budget -= passes_of(e)
            if resets_of(kind, e):
                s.resets.append((len(events) - 1, st.size, matrix_of(st.cam, st.model, s.aspect), st.bound, st.filters[st.bound]))
    s.events = events


def _pass_event(rng, s, st, name, at_least_two, room, later):
    """the pass event `name`, behind what it needs first (play_into_display: a tone mapper that has a table form); `later` pass events follow"""
    first = []
    if name == 'play_into_display' and (st.tm is None or (st.tm == 'artistic' and st.tm_sat != 1.0)):
        if room < 2:
            name = 'render'
        else:
            first = [_other_one(rng, s, st, 'tm_create')]
    return first + [_pass_one(rng, s, st, name, at_least_two, st.budget - later)]


def _other_event(rng, s, st, name, room):
    """the event `name`, behind what it needs first: a tone mapper for the tm_* events, a redirected target for target_none"""
    first = []
    if name.startswith('tm_') and name != 'tm_create' and st.tm is None:
        first = [_other_one(rng, s, st, 'tm_create')]
    if name == 'target_none' and st.target is None:
        first = [_other_one(rng, s, st, 'target')]
    if first and room < 2:
        return first
    return first + [_other_one(rng, s, st, name)]


def _pass_one(rng, s, st, name, at_least_two, budget):
    lo = 2 if at_least_two else 1
    n = int(max(1, min(budget, rng.integers(lo, 5))))
    if name == 'render':
        return {'op': 'render', 'n': n}
    if name.startswith('play_into'):
        return {'op': 'play_into_display', 'n': n} if name == 'play_into_display' else {'op': 'play_into', 'n': n, 'bucket': int(name.endswith('bucket'))}
    mode = name[5:]
    if mode in ('fused', 'frames') and s.kind == 'mcm':
        n = int(max(1, min(budget, n + (8 if mode == 'fused' and rng.uniform() < 0.5 else 0))))    # (from 8 passes on: the passes-in-registers kernel)
    return {'op': 'play', 'n': n, 'mode': mode}


def _other_one(rng, s, st, name):
    kind = s.kind
    if name == 'reset':
        return {'op': 'reset'}
    if name in ('camera', 'camera_reset'):
        hit, miss = classify(st.size[0], st.size[1], s.resets[-1][2], s.shard)
        st.cam = _mixed_camera(rng, st.size, st.model, s.shard, s.aspect) if hit and miss else _camera(rng, int(rng.integers(0, 3)))
        return {'op': 'camera', 'cam': dict(st.cam), 'reset': name == 'camera_reset'}
    if name == 'transform':
        st.model = _model(rng) if rng.uniform() < 0.5 else dict(scale=[float(v) for v in rng.uniform(0.6, 1.5, size=3)],
                                                                translation=[float(v) for v in rng.uniform(-0.15, 0.15, size=3)], angle=float(rng.uniform(-1, 1)))
        return {'op': 'transform', 'model': dict(st.model)}
    if name == 'lens':
        st.cam = dict(st.cam, fovy=float(rng.uniform(0.4, 1.5)), near=float(rng.choice([0.01, 0.1, 0.5])), far=float(rng.choice([10.0, 100.0])))
        return {'op': 'lens', 'fovy': st.cam['fovy'], 'near': st.cam['near'], 'far': st.cam['far']}
    if name == 'fused':
        st.fused = not st.fused
        return {'op': 'fused', 'value': st.fused}
    if name in ('tf_direct', 'tf_property'):
        return {'op': 'tf', 'tf': _tf(rng, channels(s.volumes[st.bound][0]) == 2), 'via': name[3:]}
    if name.startswith('env_'):
        return {'op': 'env', 'form': name[4:], 'env': _env(rng, name[4:])}
    if name == 'prop':
        names = sorted(PROPERTIES[kind])
        pname = names[int(rng.integers(0, len(names)))]
        for _ in range(16):
            value = _value(rng, kind, pname)
            if value != st.props[pname] and _props_ok(dict(st.props, **{pname: value}), False):
                break
        else:
            pname, value = 'extinction', st.props['extinction'] + 1.0      # (LAO only: every other value would be too dear)
        st.props[pname] = value
        return {'op': 'prop', 'name': pname, 'value': value}
    if name == 'filter':
        others = [f for f in FILTERS if f != st.filters[st.bound]]
        st.filters[st.bound] = others[int(rng.integers(0, 2))]
        return {'op': 'filter', 'vol': st.bound, 'filter': st.filters[st.bound]}
    if name == 'upload':
        fmt, _, texels = s.volumes[st.bound]
        dims = texels.shape[:3]
        box = tuple(int(rng.integers((n + 1) // 2, n + 1)) for n in dims)      # at least half of every axis: a box the camera cannot miss
        lo = [int(rng.integers(0, n - b + 1)) for n, b in zip(dims, box)]
        block = _texels(rng, fmt, box, False)
        if rng.uniform() < 0.5:                           # a flat block at one end of the format's range stands out from the blob around it
            flat = block.reshape(-1)
            block = np.full_like(block, flat.max() if rng.uniform() < 0.5 else flat.min())
        return {'op': 'upload', 'vol': st.bound, 'at': (lo[2], lo[1], lo[0]), 'block': block}
    if name == 'wide':
        return {'op': 'wide', 'vol': st.bound, 'value': bool(rng.integers(0, 2))}
    if name == 'set_volume':
        st.bound = [k for k in range(len(s.volumes)) if k != st.bound][int(rng.integers(0, len(s.volumes) - 1))]
        return {'op': 'set_volume', 'vol': st.bound}
    if name == 'resize':
        while True:
            size = _size(rng)
            if size != st.size:
                break
        st.size, st.target = size, None
        return {'op': 'resize', 'size': size}
    if name.startswith('option_'):
        o = name[7:]
        vals = [v for v in OPTIONS[o][1] if v != st.options[o]]
        st.options[o] = int(vals[int(rng.integers(0, len(vals)))])
        return {'op': 'option', 'option': o, 'value': st.options[o]}
    if name == 'target':
        st.target = int(rng.integers(0, 2)) if st.target is None or rng.uniform() < 0.5 else st.target      # another holder, or the same one again
        return {'op': 'target', 'to': st.target}
    if name == 'target_none':
        st.target = None
        return {'op': 'target', 'to': None}
    if name == 'tm_create':
        st.tm = TONEMAPPERS[int(rng.integers(0, len(TONEMAPPERS)))]
        st.tm_sat = 1.0
        return {'op': 'tm_create', 'kind': st.tm}
    if name == 'tm_render':
        return {'op': 'tm_render'}
    if name == 'tm_params':
        if st.tm == 'artistic':
            st.tm_sat = 1.0 if rng.uniform() < 0.6 else float(rng.uniform(0.2, 1.6))
            values = {'low': float(rng.uniform(0, 0.2)), 'high': float(rng.uniform(0.6, 1.5)), 'mid': float(rng.uniform(0.2, 0.8)),
                      'saturation': st.tm_sat, 'gamma': float(rng.choice([1.0, 2.2]))}
        elif st.tm == 'range':
            values = {'min': float(rng.uniform(0, 0.3)), 'max': float(rng.uniform(0.5, 2.0)), 'gamma': float(rng.choice([1.0, 2.2]))}
        else:
            values = {'exposure': float(rng.uniform(0.3, 3.0)), 'gamma': float(rng.choice([1.0, 2.2]))}
        return {'op': 'tm_params', 'values': values}
    if name in ('tm_fuse', 'tm_table'):
        return {'op': 'tm_option', 'option': name[3:], 'value': int(rng.integers(0, 2 if name == 'tm_fuse' else 3))}
    if name == 'tm_destroy':
        st.tm = None
        return {'op': 'tm_destroy'}
    if name in ('read', 'read_twice'):
        pool = ['render', 'accum'] if kind != 'mcm' else ['render', 'position', 'direction', 'transmittance', 'radiance']
        pick = [b for b in pool if rng.uniform() < 0.5] or [pool[-1]]
        return {'op': 'read', 'buffers': pick, 'twice': name == 'read_twice'}
    if name == 'sample_count':
        return {'op': 'sample_count'}
    raise KeyError(name)


def life(kind, seed):
    return setup(kind, seed).events


def without(s, index):
    """the twin of a life: the same life with event `index` left out — a plain reset in its place if it resets, so that the passes accumulate
    and the renderer draws as in the life itself and only what the event set is missing (a copy; the drawn life is not changed)"""
    t = types.SimpleNamespace(**vars(s))
    t.events = [e if i != index else {'op': 'reset'} for i, e in enumerate(s.events) if i != index or resets_of(s.kind, e)]
    return t


def hit_miss_at(kind, seed, reset_index):
    """(HIT tiles, MISS tiles) the host's classification gives for the matrix, size and shard in force at the life's reset `reset_index`
    (0: the one before the first event)"""
    s = setup(kind, seed)
    _, size, m, _, _ = s.resets[reset_index]
    return classify(size[0], size[1], m, s.shard)


def armed(kind, seed):
    """[(event index, what it perturbs)] of the perturbing events in the armed position: after a reset at which both tile classes exist,
    behind at least 2 fused passes under that reset's matrix, and with at least 2 more passes before the next reset"""
    s = setup(kind, seed)
    out = []
    reset, fused, passes, still = 0, True, 0, True          # the reset in force, r.fused, fused passes since it, its matrix still in force
    for i, e in enumerate(s.events):
        op = e['op']
        if op in PERTURBING and not resets_of(kind, e) and still and passes >= 2 and min(hit_miss_at(kind, seed, reset)) > 0:
            after = 0
            for f in s.events[i + 1:]:
                if resets_of(kind, f):
                    break
                after += passes_of(f)
            if after >= 2:
                out.append((i, PERTURBING[op], reset))
        if op == 'fused':
            fused = e['value']
        if op in ('camera', 'transform', 'lens'):
            still = False
        if op in PASS_OPS and (fused or op != 'render'):
            passes += e['n']
        if resets_of(kind, e):
            reset, passes, still = reset + 1, 0, True
    return out


def engaging_seeds(kind, count=3):
    """the first default seeds whose life reaches the armed position in the plainest way: under a reset at which an R8 volume is bound with
    the LINEAR filter, with two render() calls into the renderer's own buffer as the first passes since that reset, and with no option, no
    environment map other than an opaque 1x1 one and no redirected target before.  There the tile classes must be in force on the device:
    tile_classes() reports both classes (for the ray marchers from the second fused pass on)."""
    out = []
    for seed in range(*DEFAULT_SEEDS):
        s = setup(kind, seed)
        if s.env is not None and (s.env.shape[:2] != (1, 1) or s.env.dtype != np.uint8 or s.env[0, 0, 3] != 255):
            continue
        for i, _, reset in armed(kind, seed):
            if kind == 'lao':                             # (no tile classes to engage: any life in the armed position)
                out.append(seed)
                break
            at = s.resets[reset][0]                      # the event that reset (-1: the first reset)
            before = s.events[:i]
            first_pass = next((e for e in s.events[at + 1:i] if e['op'] in PASS_OPS), None)
            fused = True
            for e in s.events[:at + 1]:
                fused = e['value'] if e['op'] == 'fused' else fused
            if s.volumes[s.resets[reset][3]][0] == 'R8' and s.resets[reset][4] == 'linear' and fused and first_pass is not None \
                    and first_pass['op'] == 'render' and first_pass['n'] >= 2 \
                    and not any(e['op'] in ('option', 'env', 'target', 'play_into', 'play_into_display', 'fused', 'filter') for e in before):
                out.append(seed)
                break
        if len(out) == count:
            break
    return out


def owed(kind, seed):
    """the index of an MCM life's float / half environment event that comes while the settled MISS kernel's samples are still owed, or None.
    By what include/vpt.h says of VPT_OPTION_SETTLED_MISS: a white 1x1 environment since the construction, an R8 volume with the LINEAR
    filter, both tile classes at the reset in force, the options as they are by default, no tone mapper armed, no redirected target, the
    reset's matrix still in force, two render() calls as the event's direct predecessor, and state checks after the last event only (a read of
    the radiance buffer is the catch-up)."""
    s = setup(kind, seed)
    if kind != 'mcm' or not s.lazy or s.fast or s.env is not None or s.split == 1:
        return None
    reset, fused, still, clean = 0, True, True, True
    for i, e in enumerate(s.events):
        op = e['op']
        if op == 'env':
            prev = s.events[i - 1] if i else None
            if e['form'] in ('float', 'half3x2') and clean and still and fused and prev and prev['op'] == 'render' and prev['n'] >= 2 \
                    and min(hit_miss_at(kind, seed, reset)) > 0 and s.volumes[s.resets[reset][3]][0] == 'R8' and s.resets[reset][4] == 'linear' \
                    and not any(f['op'] == 'filter' for f in s.events[s.resets[reset][0] + 1:i]):
                return i
            clean = False
        if op in ('option', 'target', 'play_into', 'play_into_display', 'tm_render', 'wide', 'upload'):
            clean = False
        if op == 'fused':
            fused = e['value']
        if op in ('camera', 'transform', 'lens'):
            still = False
        if resets_of(kind, e):
            reset, still = reset + 1, True
    return None


# ---- the script --------------------------------------------------------------------------------------------------------------------
def _short(v):
    if isinstance(v, np.ndarray):
        return "<%s %s>" % (v.dtype, "x".join(str(n) for n in v.shape))
    if isinstance(v, float):
        return "%.4g" % v
    if isinstance(v, dict):
        return "{%s}" % ", ".join("%s: %s" % (k, _short(x)) for k, x in v.items())
    if isinstance(v, (list, tuple)):
        return "[%s]" % ", ".join(_short(x) for x in v)
    return repr(v)


def describe(kind, seed, s=None):
    s = s or setup(kind, seed)
    lines = ["# life %s seed %d: image %dx%d, shard %s, fast_math %s, %s state checks, destroyed early: %s" % (
        kind, seed, s.size[0], s.size[1], s.shard, s.fast, "last" if s.lazy else "all", s.early)]
    for k, (fmt, filt, texels) in enumerate(s.volumes):
        lines.append("v%d = Volume(%s, %s, %s)" % (k, fmt, "x".join(str(n) for n in texels.shape[:3]), filt))
    lines.append("r = %s(v0, camera(%s), env=%s, model=%s)" % (kind, _short(s.cam), _short(s.env), _short(s.model)))
    if s.tf is not None:
        lines.append("r.setTransferFunction(%s)" % _short(s.tf))
    lines.append("r.<properties> = %s" % _short(s.props))
    lines.append("r.reset()")
    for i, e in enumerate(s.events):
        lines.append("%2d: %s(%s)" % (i, e['op'], ", ".join("%s=%s" % (k, _short(v)) for k, v in e.items() if k != 'op')))
    return "\n".join(lines)
