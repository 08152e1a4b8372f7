"""CPU: the conditions the drawn renderer lives (tests/renderer_life_cases.py) must meet for tests/test_gpu_renderer_life.py to check
what it is there for.  These are conditions on the drawn inputs, not measurements: where one fails, the generator's draws are what
changes, not the thresholds.  VPT_LIFE_SEEDS=a:b widens the set of seeds."""
import hashlib
import os
import time

import numpy as np
import pytest

import renderer_life_cases as L
from test_gpu_fuzz import oracle_only
from test_gpu_renderer_life import oracle_side

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_LIFE_SEEDS", "%d:%d" % L.DEFAULT_SEEDS).split(":")])
LIVES = [(kind, seed) for kind in L.KINDS for seed in _SEEDS]
ARMED = ('tf', 'env', 'matrix', 'filter', 'upload_block', 'option', 'target', 'tone mapper', 'fused toggle')


def digest(s):
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, np.ndarray):
            h.update(str((v.dtype, v.shape)).encode()); h.update(np.ascontiguousarray(v).tobytes())
        elif isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode()); feed(v[k])
        elif isinstance(v, (list, tuple)):
            for x in v:
                feed(x)
        else:
            h.update(repr(v).encode())
    feed([s.size, s.shard, s.cam, s.model, s.volumes, s.tf, s.env, s.props, s.fast, s.lazy, s.early, s.split, s.start, s.events, s.resets])
    return h.hexdigest()


def test_generation_repeats_itself_byte_for_byte_and_is_quick():
    L.setup.cache_clear()
    t0 = time.perf_counter()
    first = [digest(L.setup(k, s)) for k, s in LIVES]
    took = time.perf_counter() - t0
    scripts = [L.describe(k, s) for k, s in LIVES]
    L.setup.cache_clear()
    assert [digest(L.setup(k, s)) for k, s in LIVES] == first
    assert [L.describe(k, s) for k, s in LIVES] == scripts
    assert took < 30.0 * max(1, len(_SEEDS) // 24), "%.1f s to draw %d lives" % (took, len(LIVES))


def test_the_sizes_are_the_smallest_at_which_the_machinery_engages():
    for kind, seed in LIVES:
        s = L.setup(kind, seed)
        sizes = [s.size] + [e['size'] for e in s.events if e['op'] == 'resize']
        assert all(33 <= w <= 112 and 17 <= h <= 96 for w, h in sizes), (kind, seed, sizes)
        for fmt, filt, texels in s.volumes:
            assert max(texels.shape[:3]) <= 24 and len(set(texels.shape[:3])) > 1 and texels.dtype == L.DTYPES[fmt], (kind, seed, fmt, texels.shape)
        assert 6 <= len(s.events) <= 12 and sum(L.passes_of(e) for e in s.events) <= L.MAX_PASSES, (kind, seed)
        assert (s.shard is not None) == (seed % 3 == 1)
        assert len(s.resets) == 1 + sum(L.resets_of(kind, e) for e in s.events)


@pytest.mark.parametrize("kind", L.KINDS)
def test_every_event_of_the_alphabet_occurs_three_times(kind):
    count = {name: 0 for name in L.entries(kind) + L.pass_entries(kind)}
    for seed in _SEEDS:
        for e in L.life(kind, seed):
            count[L.entry_of(e)] += 1
    assert not {n: c for n, c in count.items() if c < 3}, count
    assert sum(1 for seed in _SEEDS if L.setup(kind, seed).fast) == (len(_SEEDS) // 4 if kind == 'mcm' else 0)


@pytest.mark.parametrize("kind", L.KINDS)
def test_every_perturbing_event_occurs_twice_in_the_armed_position(kind):
    count = {what: 0 for what in ARMED if what != 'env' or kind in L.ENV_KINDS}
    for seed in _SEEDS:
        for _, what, _ in L.armed(kind, seed):
            count[what] += 1
    assert not {n: c for n, c in count.items() if c < 2}, count
    assert len(L.engaging_seeds(kind)) == 3


def test_mcm_lives_set_a_float_and_a_half_map_while_settled_samples_are_owed():
    """the catch-up of vpt_renderer_set_environment_texels has something to catch up with in two default lives at least, one per texel format"""
    forms = [L.life('mcm', seed)[L.owed('mcm', seed)]['form'] for seed in range(*L.DEFAULT_SEEDS) if L.owed('mcm', seed) is not None]
    assert 'float' in forms and 'half3x2' in forms, forms


def test_drawing_inside_oracle_only_gives_the_same_lives(oracle):
    want = [digest(L.setup('mcm', seed)) for seed in range(6)]
    L.setup.cache_clear()
    with oracle_only():
        got = [digest(L.setup('mcm', seed)) for seed in range(6)]
    assert got == want


def test_most_lives_see_both_tile_classes_and_few_are_one_tile():
    both = one = 0
    for kind, seed in LIVES:
        s = L.setup(kind, seed)
        classes = [L.hit_miss_at(kind, seed, k) for k in range(len(s.resets))]
        both += any(hit > 0 and miss > 0 for hit, miss in classes)
        one += any(hit + miss == 1 for hit, miss in classes)
    assert both >= 0.6 * len(LIVES), (both, len(LIVES))
    assert one <= 0.1 * len(LIVES), (one, len(LIVES))


@pytest.mark.parametrize("kind", L.KINDS)
def test_every_format_is_bound_twice_and_every_filter_in_force_for_three_passes(kind):
    bound = {f: 0 for f in L.FORMATS}
    passes = {f: 0 for f in L.FILTERS}
    special = 0
    for seed in _SEEDS:
        s = L.setup(kind, seed)
        vol, filters = 0, [v[1] for v in s.volumes]
        bound[s.volumes[0][0]] += 1
        for e in s.events:
            if e['op'] == 'set_volume':
                vol = e['vol']
                bound[s.volumes[vol][0]] += 1
                special += bool(s.volumes[vol][0] == 'R32F' and not np.isfinite(s.volumes[vol][2]).all())
            elif e['op'] == 'filter':
                filters[e['vol']] = e['filter']
            passes[filters[vol]] += L.passes_of(e)
    assert min(bound.values()) >= 2, bound
    assert min(passes.values()) >= 3, passes


_oracle_runs = {}


def oracle_runs(oracle):
    """(seconds of every life's oracle side on one thread, [(kind, seed, event index, op, image differs)] of every twin), computed once"""
    if not _oracle_runs:
        seconds, twins = {}, []
        for kind, seed in LIVES:                               # (drawn with the real library: classify() holds it, and so does the cache from here on)
            L.setup(kind, seed)
        with oracle_only():
            for kind, seed in LIVES:
                s = L.setup(kind, seed)
                t0 = time.perf_counter()
                image = oracle_side(oracle, s).image
                seconds[kind, seed] = time.perf_counter() - t0
                for i, e in enumerate(s.events):
                    if e['op'] in L.VISIBLE:
                        twin = oracle_side(oracle, L.without(s, i), nthreads=4).image
                        twins.append((kind, seed, i, e['op'], image.shape != twin.shape or bool((image != twin).any())))
        _oracle_runs['seconds'], _oracle_runs['twins'] = seconds, twins
    return _oracle_runs['seconds'], _oracle_runs['twins']


def test_the_oracle_side_of_a_life_takes_under_three_seconds(oracle):
    seconds, _ = oracle_runs(oracle)
    slow = {k: round(v, 2) for k, v in seconds.items() if v >= 3.0}
    assert not slow, slow


def test_perturbations_are_visible(oracle):
    """a life without one of its TF / env / filter / upload_block / setVolume / property events ends in another image in at least 80 % of
    the (life, event) pairs: a stale table would change what the device test compares"""
    _, twins = oracle_runs(oracle)
    differ = sum(1 for t in twins if t[4])
    assert len(twins) >= len(LIVES) and differ >= 0.8 * len(twins), (differ, len(twins), [t[:4] for t in twins if not t[4]])
