"""The scenario table of tests/stream_order_worker.py (tests/test_gpu_stream_order.py runs it on the GPU): what it must hold whatever the
scenarios do.  Reads the table only: no GPU, no torch."""
import stream_order_worker as S

# the entries that wait for the host by design: host uploads, the tables, a float volume's finalize, multi-pass rank and smooth, the
# filtered resample, every query and read-back (the voxel fields' labelling and transform read counts back, the graph's two labellings too)
MUST_BLOCK = {'upload_block', 'setTransferFunction', 'set_environment', 'set_environment_texels', 'finalize(float)', 'smooth(n)', 'rank(n)',
              'resample(filtered)', 'read', 'components', 'distance', 'graph'}
# the entries include/vpt.h lists as returning without a host wait: each needs a scenario that finds the gate closed behind it
MUST_NOT_BLOCK = {'upload_block_device', 'finalize', 'reduce', 'smooth(1)', 'rank(1)', 'combine', 'window', 'derive_gradient', 'resample(nearest)',
                  'render', 'play_into', 'play_into_display', 'set_render_target', 'join'}


def test_the_table_is_plain_data_around_callables():
    assert S.SCENARIOS and all(callable(s['fn']) and isinstance(s['params'], dict) for s in S.SCENARIOS)


def test_names_are_unique():
    names = [s['name'] for s in S.SCENARIOS]
    assert len(names) == len(set(names))


def test_every_scenario_is_asynchronous_or_blocking():
    assert all(s['waits'] in ('asynchronous', 'blocking') for s in S.SCENARIOS)


def test_every_entry_is_a_known_one_and_the_lists_are_disjoint():
    assert MUST_BLOCK <= set(S.BLOCKING_ENTRIES) and MUST_NOT_BLOCK <= set(S.ASYNC_ENTRIES)
    assert not set(S.BLOCKING_ENTRIES) & set(S.ASYNC_ENTRIES)
    known = set(S.BLOCKING_ENTRIES) | set(S.ASYNC_ENTRIES)
    for s in S.SCENARIOS:
        assert s['entries'] and set(s['entries']) <= known, s['name']


def test_blocking_entries_appear_in_blocking_scenarios_only():
    for s in S.SCENARIOS:
        blocking = set(s['entries']) & set(S.BLOCKING_ENTRIES)
        if s['waits'] == 'asynchronous':
            assert not blocking, (s['name'], blocking)
        else:
            assert blocking, "%s is marked blocking but lists no entry that waits" % s['name']


def test_every_asynchronous_entry_has_a_scenario_that_looks_at_the_gate():
    seen = set()
    for s in S.SCENARIOS:
        if s['waits'] == 'asynchronous':
            seen |= set(s['entries'])
    assert set(S.ASYNC_ENTRIES) <= seen, set(S.ASYNC_ENTRIES) - seen


def test_every_family_is_present():
    assert {s['family'] for s in S.SCENARIOS} == set('ABCDEFG') == set(S.FAMILIES)
    assert all(s['name'].startswith(s['family'] + '_') for s in S.SCENARIOS)


def test_the_graph_is_reached_on_a_callers_stream():
    (s,) = [s for s in S.SCENARIOS if 'graph' in s['entries']]
    assert s['family'] == 'C' and s['waits'] == 'blocking' and {'graph', 'graph.prune', 'upload_block_device', 'render'} <= set(s['entries'])
    # the emitters of a graph built before the gate are looked at behind it; include/vpt.h does not list them among the entries that
    # return without a host wait, so MUST_NOT_BLOCK does not name them
    (s,) = [s for s in S.SCENARIOS if 'graph.classes' in s['entries']]
    assert s['family'] == 'C' and s['waits'] == 'asynchronous' and {'graph.branch_components', 'label', 'upload_block_device'} <= set(s['entries'])
    assert not {'graph.classes', 'graph.branch_components', 'label'} & MUST_NOT_BLOCK


def test_the_gate_is_ten_enqueue_times_and_under_half_a_second():
    gate_ms = S.GATE_CYCLES * S.GATE_MS_PER_CYCLE
    assert 10.0 * S.LONGEST_ENQUEUE_MS <= gate_ms < 500.0
