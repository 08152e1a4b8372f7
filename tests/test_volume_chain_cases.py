"""The drawn volume chains (tests/volume_chain_cases.py) at the default seeds, held to the conditions without which
tests/test_gpu_volume_chain_fuzz.py could pass while checking little.  No device: numpy and the vpt_amd statements only.

The first tests hold for the whole set.  Those from ``test_the_first_seeds_are_drawn_by_the_first_rules`` on are about the seeds of the
later rules (128 ..): that the thinning steps make several passes and cross a word and a tile along x, that the thickness steps list more
centre tiles than one step of the walk takes and hold a ball that reaches past the neighbouring tile, that reconstructions propagate and
clamp, that watersheds split and a basin crosses tiles, that a block of the measuring kernel holds more ranks than its table has slots, and
that every forced slow path occurs.  The counts come from each step's 'facts', taken from the statements when the step was drawn."""
import hashlib
import time

import numpy as np

import volume_chain_cases as V

SEEDS = list(V.default_seeds())
_START = time.perf_counter()
CHAINS = {seed: V.chain(seed) for seed in SEEDS}
GENERATION_SECONDS = time.perf_counter() - _START
STEPS = [(seed, i, s) for seed in SEEDS for i, s in enumerate(CHAINS[seed]) if s['op'] != 'source']
PRODUCING = [(seed, i, s) for seed, i, s in STEPS if s['out'] is not None]


def test_generation_is_quick_and_repeats_itself():
    assert GENERATION_SECONDS < 30.0, "%.1f s for %d chains" % (GENERATION_SECONDS, len(SEEDS))
    for seed in SEEDS[:6] + SEEDS[V.LATER_SEEDS:V.LATER_SEEDS + 6] + SEEDS[V.GRAPH_SEEDS:V.GRAPH_SEEDS + 6]:
        again = V._build(seed)
        assert len(again) == len(CHAINS[seed])
        for a, b in zip(again, CHAINS[seed]):
            assert a['op'] == b['op'] and a['src'] == b['src'] and a['out'] == b['out']
            if isinstance(a['expect'], np.ndarray):
                assert a['expect'].tobytes() == b['expect'].tobytes()
            else:
                assert a['expect'] == b['expect']


def test_chains_have_the_drawn_form():
    for seed in SEEDS:
        steps = CHAINS[seed]
        assert steps[0]['op'] == 'source' and 3 <= len(steps) - 1 <= 6, seed
        d, h, w = steps[0]['shape']
        assert d * h * w <= V.MAX_VOXELS and ((d, h, w) == (1, 1, 1)) == (seed % 16 == 0), seed
        volumes = 1
        for s in steps[1:]:
            assert s['format'] in V.LEGAL[s['op']], (seed, s['op'], s['format'])
            assert s['src'] < volumes
            if s['out'] is not None:
                assert s['out'] == volumes and isinstance(s['expect'], np.ndarray) and s['expect'].size <= V.MAX_VOXELS * 2
                volumes += 1
            if s['op'] == 'resample':
                assert s['shape'][0] * s['shape'][1] * s['shape'][2] <= V.MAX_VOXELS
        text = V.describe(seed)
        assert text.count('\n') == len(steps) and 'Volume.from_array' in text


def test_few_results_are_constant():
    judged = [(seed, i, s) for seed, i, s in PRODUCING if s['expect'].size > 1 and np.prod(s['shape']) > 1]
    constant = [(seed, i, s['op']) for seed, i, s in judged if V._constant(s['expect'])]
    assert len(judged) >= 100
    assert len(constant) <= 0.02 * len(judged), "%d of %d volume-producing steps give a constant volume: %s" % (len(constant), len(judged), constant)


def test_every_operation_occurs_three_times():
    count = {entry: 0 for entry in V.ENTRIES + V.GRAPH_ENTRIES}
    for _, _, s in STEPS:
        count[(s['op'], s['sub'])] += 1
    rare = {entry: n for entry, n in count.items() if n < 3}
    assert not rare, rare


def test_every_legal_format_meets_every_operation():
    seen = {(s['format'], s['op']) for _, _, s in STEPS}
    missing = [(fmt, op) for op, formats in V.LEGAL.items() for fmt in formats if (fmt, op) not in seen]
    assert not missing, missing
    modes = {(s['format'], s['kwargs']['mode']) for _, _, s in STEPS if s['op'] == 'resample'}
    missing = [(fmt, mode) for fmt in V.FORMATS for mode in ('nearest', 'filtered') if (mode == 'nearest' or fmt in V.RESAMPLE_FILTERED) and (fmt, mode) not in modes]
    assert not missing, missing
    windows = {(s['format'], s['kwargs']['format']) for _, _, s in STEPS if s['op'] == 'window'}
    assert {fmt for fmt, _ in windows} == set(V.LEGAL['window']) and {bits for _, bits in windows} == {'r8', 'r16'}


def shapes_of(family):
    return [s['shape'] for _, _, s in STEPS if V.FAMILY.get(s['op']) == family]


def test_every_family_sees_its_tile_edges_on_every_axis():
    """No extent is ruled out by the voxel cap: the condition is per axis, the largest extent is 257, and the other two axes may be 1."""
    missing = []
    for family, tile in V.TILES.items():
        shapes = shapes_of(family)
        for axis, name in ((2, 'x'), (1, 'y'), (0, 'z')):
            for extent in V.tile_extents(tile[2 - axis], V.WORD.get((family, name))):
                if not any(shape[axis] == extent for shape in shapes):
                    missing.append((family, name, extent))
    assert not missing, missing


def test_both_forms_of_every_vector_kernel_run():
    for family in V.VECTOR_FAMILIES + ('resample',):
        widths = [shape[2] for shape in shapes_of(family)]
        for modulus in (4, 32):
            assert any(w % modulus == 0 for w in widths) and any(w % modulus for w in widths), (family, modulus)
    widths = [s['shape'][2] for _, _, s in STEPS if s['op'] == 'reduce']
    for modulus in (4, 32):
        assert any(w % modulus == 0 for w in widths) and any(w % modulus for w in widths), ('reduce', modulus)
    for op in ('window', 'combine'):                              # 16-byte groups of the whole volume: a last partial group or none
        voxels = [int(np.prod(s['shape'])) for _, _, s in STEPS if s['op'] == op]
        assert any(n % 16 == 0 for n in voxels) and any(n % 16 for n in voxels), op


def test_every_source_of_a_second_volume_occurs():
    for op in ('combine', 'compare'):
        seen = {s['b_source'] for _, _, s in STEPS if s['op'] == op}
        assert seen == set(V.B_SOURCES), (op, seen)
    mixed = [s for _, _, s in STEPS if s['op'] == 'combine' and s['b_source'] == 'other_width']
    assert all(s['sub'] == 'mask' for s in mixed)
    assert any(s['kwargs']['b'][0] == 'volume' and s['b_source'] == 'rg_channel' for _, _, s in STEPS if s['op'] in ('combine', 'compare'))


def test_blocks_are_uploaded_between_derive_steps():
    between = 0
    for seed in SEEDS:
        steps = CHAINS[seed]
        for i, s in enumerate(steps):
            if s['op'] == 'upload_block' and any(t['out'] is not None for t in steps[1:i]) and \
                    any(t['out'] is not None and t['src'] == s['src'] for t in steps[i + 1:]):
                between += 1
    assert between >= 10, between


def test_a_float_source_holds_the_special_values():
    found = [seed for seed in SEEDS if CHAINS[seed][0]['kwargs']['texels'].dtype == np.float32 and
             np.isnan(CHAINS[seed][0]['kwargs']['texels']).any() and np.isinf(CHAINS[seed][0]['kwargs']['texels']).any()]
    assert found
    assert any(np.signbit(CHAINS[seed][0]['kwargs']['texels'][CHAINS[seed][0]['kwargs']['texels'] == 0]).any() for seed in found)
    outside = [seed for seed in SEEDS if CHAINS[seed][0]['kwargs']['texels'].dtype == np.float32 and int(np.prod(CHAINS[seed][0]['shape'])) >= 1000]
    assert outside
    for seed in outside:
        t = CHAINS[seed][0]['kwargs']['texels']
        finite = t[np.isfinite(t)]
        assert (finite < 0).any() and (finite > 1).any(), seed


# ---- the later units: every count below is of the drawn set, taken from the statements when the step was drawn (its 'facts') ------------
LATER_STEPS = [(seed, i, s) for seed, i, s in STEPS if s['op'] in V.LATER]


def facts_of(family):
    return [s['facts'] for _, _, s in LATER_STEPS if V.FAMILY[s['op']] == family]


def test_the_first_seeds_are_drawn_by_the_first_rules():
    for seed in SEEDS[:V.LATER_SEEDS]:
        assert all(s['op'] in V.OLD_OPS + ('source',) for s in CHAINS[seed]), seed
    assert len(SEEDS) % 16 == 0 and SEEDS[0] == 0 and len(SEEDS) > V.LATER_SEEDS
    for seed in SEEDS[V.LATER_SEEDS:V.GRAPH_SEEDS]:
        assert not any(s['op'] in V.GRAPH for s in CHAINS[seed]), seed


def chains_digest(seeds):
    h = hashlib.sha256()
    for seed in seeds:
        for s in CHAINS[seed]:
            h.update(repr((s['op'], s['sub'], s['src'], s['out'], s['shape'], s['format'])).encode())
            e = s['expect']
            h.update(np.ascontiguousarray(e).tobytes() if isinstance(e, np.ndarray) else repr(e).encode())
    return h.hexdigest()


def test_the_chains_before_the_graph_rules_are_what_they_were():
    """every step's operation, volumes, shape, format and expected bytes of seeds 0 .. 127 and 128 .. 223, as they were drawn before the
    graph rules joined (the digests were taken from the file as it was then)"""
    assert chains_digest(SEEDS[:V.LATER_SEEDS]) == '028619680012038586cbcde812576811ed7d9fe13303d3a6e646c6a254f84727'
    assert chains_digest(SEEDS[V.LATER_SEEDS:V.GRAPH_SEEDS]) == '729049973b01db6e17a77b1a8cf9dea0013a862ca36d4b2e6eb3e954a37c8dc8'


def test_a_later_chain_has_two_later_steps_and_one_reads_a_derived_volume():
    for seed in SEEDS[V.LATER_SEEDS:V.GRAPH_SEEDS]:
        later = [s for s in CHAINS[seed][1:] if s['op'] in V.LATER]
        assert len(later) >= 2 and any(V._reads_derived(s) for s in later), seed
        for s in later:
            if V.FAMILY[s['op']] in V.SLOW_FAMILIES:
                assert int(np.prod(s['shape'])) <= V.SLOW_VOXELS, (seed, s['op'], s['shape'])
    # a skeleton, a thickness pair and a reconstruction each stand in front of another derive step
    for family in ('skeleton', 'thickness', 'reconstruct'):
        read = 0
        for seed in SEEDS[V.LATER_SEEDS:]:
            steps = CHAINS[seed]
            made = {s['out'] for s in steps[1:] if s['out'] is not None and V.FAMILY.get(s['op']) == family and s['op'] in V.LATER}
            read += sum(1 for s in steps[1:] if s['out'] is not None and s['src'] in made)
        assert read >= 10, (family, read)


def test_the_thinning_steps_thin():
    facts = facts_of('skeleton')
    assert len(facts) >= 20
    assert 2 * sum(f['passes'] >= 3 for f in facts) >= len(facts)
    assert 2 * sum(0 < f['kept_voxels'] < f['object_voxels'] for f in facts) >= len(facts)
    assert sum(f['both_tiles'] for f in facts) >= 3
    wide = {s['facts']['mode'] for _, _, s in LATER_STEPS if V.FAMILY[s['op']] == 'skeleton' and s['shape'][2] > 32}
    assert wide == set(V.SKELETON_MODES), wide


def test_the_thickness_steps_walk_and_reach():
    facts = facts_of('thickness')
    assert len(facts) >= 20
    assert 2 * sum(f['differs_from_distance'] for f in facts) >= len(facts)
    assert sum(f['centre_tiles'] > 64 for f in facts) >= 2 and sum(f['centre_tiles'] > 128 for f in facts) >= 1      # a second and a third step of the walk
    assert sum(f['largest_in_a_tile'] > 64 for f in facts) >= 1                                                  # a ball past the neighbouring tile
    for key in ('seeds', 'steps'):
        assert len({s['kwargs'][key] for _, _, s in LATER_STEPS if s['op'] == 'thickness'}) == {'seeds': 2, 'steps': 4}[key], key


def test_the_reconstructions_propagate():
    facts = [s['facts'] for _, _, s in LATER_STEPS if s['op'] == 'reconstruct']
    assert len(facts) >= 10
    assert 2 * sum(f['differs_from_both'] for f in facts) >= len(facts), (sum(f['differs_from_both'] for f in facts), len(facts))
    assert sum(f['marker_not_under_mask'] for f in facts) >= 3
    assert {s['b_source'] for _, _, s in LATER_STEPS if s['op'] == 'reconstruct'} == set(V.B_SOURCES[:4])
    geodesic = [s for _, _, s in LATER_STEPS if s['op'] == 'geodesic' and s['sub'] in V.TAKES_H]
    assert any(s['kwargs']['h'] == 0 for s in geodesic) and any(s['facts']['h_above_range'] for s in geodesic)
    assert {s['kwargs']['channel'] for _, _, s in LATER_STEPS if s['op'] == 'geodesic'} == {0, 1}


def test_the_watersheds_split():
    steps = [s for _, _, s in LATER_STEPS if s['op'].startswith('basins_')]
    assert len(steps) >= 20
    assert 2 * sum(s['facts']['listed'] >= 2 for s in steps) >= len(steps)
    assert sum(s['facts']['spans_tiles'] for s in steps) >= 3
    assert {s['kwargs']['polarity'] for s in steps} == {'minima', 'maxima'}
    assert sum(s['kwargs']['texels'] is not None for s in steps) >= 3
    assert any(s['kwargs']['texels'] is not None and s['kwargs']['texels'][0] == 'volume' for s in steps)
    assert {s['kwargs']['channel'] for s in steps} == {0, 1}


def test_the_measuring_table_overflows_and_values_are_derived():
    steps = [s for _, _, s in LATER_STEPS if s['op'] in ('measure', 'basins_measure')]
    assert any(s['facts']['block_ranks'] > 512 for s in steps), max(s['facts']['block_ranks'] for s in steps)       # MS_SLOTS
    assert any(s['facts'].get('values_of_a_derived_pair') for s in steps)
    assert any(s['kwargs']['b'] is None for s in steps) and any(s['kwargs']['first'] > 0 for s in steps) and any(s['kwargs']['n'] is not None for s in steps)
    sets = [s['kwargs']['ranks'] for _, _, s in LATER_STEPS if s['op'] in ('keep_set', 'basins_keep_set')]
    assert any(isinstance(r, np.ndarray) for r in sets)
    lists = [r for r in sets if isinstance(r, tuple) and r]
    assert any(len(set(r)) < len(r) for r in lists) and any(max(r) > (1 << 32) for r in lists)


def test_every_forced_slow_path_occurs_three_times():
    count = {(family, hook): 0 for family, hooks in V.FORCED.items() for hook in hooks}
    for _, _, s in LATER_STEPS:
        if s['forced'] is not None:
            count[(V.FAMILY[s['op']], s['forced'])] += 1
    assert all(n >= 3 for n in count.values()), count


# ---- the graph rules (seeds 224 ..) ------------------------------------------------------------------------------------------------
GRAPH_STEPS = [(seed, i, s) for seed, i, s in STEPS if s['op'] in V.GRAPH]


def test_the_graph_seeds_reach_the_graph_behind_other_steps():
    assert len(SEEDS) == V.GRAPH_SEEDS + 32 and all(seed >= V.GRAPH_SEEDS for seed, _, _ in GRAPH_STEPS)
    for seed in SEEDS[V.GRAPH_SEEDS:]:
        mine = [s for s in CHAINS[seed][1:] if s['op'] in V.GRAPH]
        assert len(mine) >= 2 and any(V._reads_derived(s) for s in mine), seed
        assert all(int(np.prod(s['shape'])) <= V.SLOW_VOXELS for s in mine), seed
    count = {op: 0 for op in V.GRAPH}
    for _, _, s in GRAPH_STEPS:
        count[s['op']] += 1
    assert all(n >= 2 for n in count.values()), count
    # a class pair stands in front of another step (two-channel steps and the 2-D transfer function follow it), and is a chain's last volume
    read = last = 0
    for seed in SEEDS[V.GRAPH_SEEDS:]:
        steps = CHAINS[seed]
        made = {s['out'] for s in steps[1:] if s['op'] == 'graph_classes'}
        read += sum(1 for s in steps[1:] if s['src'] in made)
        last += max(s['out'] for s in steps if s['out'] is not None) in made
    assert read >= 2 and last >= 1, (read, last)
    assert {s['kwargs']['via'] for _, _, s in GRAPH_STEPS if s['op'] != 'centreline_prune'} == {'skeleton', 'range'}
    assert {s['kwargs']['prune_rounds'] for _, _, s in GRAPH_STEPS if s['op'] == 'centreline_prune'} == {1, 3}


def test_the_drawn_prunings_drop_a_spur_and_keep_one():
    prunes = [s for _, _, s in GRAPH_STEPS if s['op'] == 'graph_prune']
    assert len(prunes) >= 8
    assert 2 * sum(s['facts']['spur_dropped'] and s['facts']['spur_kept'] for s in prunes) >= len(prunes)
    assert any(s['kwargs']['debris'] for s in prunes) and any(not s['kwargs']['debris'] for s in prunes)
    assert any(s['kwargs']['weights'] != (10, 14, 17) for s in prunes) and any(s['kwargs']['fill'] for s in prunes)
    lines = [s for _, _, s in GRAPH_STEPS if s['op'] == 'centreline_prune']
    assert 2 * sum(s['facts']['differs_from_unpruned'] for s in lines) >= len(lines), [s['facts'] for s in lines]
    graphs = [s['facts'] for _, _, s in GRAPH_STEPS if s['op'] != 'centreline_prune']
    assert 2 * sum(f['branches'] >= 3 and f['nodes'] >= 1 for f in graphs) >= len(graphs)
    windows = [s['kwargs'] for _, _, s in GRAPH_STEPS if s['op'] == 'graph_branches']
    assert any(k['first'] > 0 for k in windows) and any(k['n'] is not None for k in windows)
