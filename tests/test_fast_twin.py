"""CPU: the float64 twin of the MCM fast-arithmetic variant (oracle/vpt_oracle.c vpo_mcm_fast64: the same PCG stream, algebraic forms and
branches as vpt_kernels_mcm.h's mcm_events_fast / fast_path_end / sample_hg_fast / photon_start_fast, in double) against the CONTRACT
oracle, with which it agrees algebraically: this validates the twin without a GPU and measures A_REF, the slack that float32 arithmetic of
the contract's quality needs (tests/fast_twin_cases.py: the cases, the rule).  Teacher-forced on the oracle's own
trajectories: every pass, vpo_mcm_integrate and the twin start from the same copy of the oracle's state.

Asserted at slack A_REF: no robust pixel-event disagrees; at most 1 % of a case's pixel-events and 0.1 % of all are fragile; each of the
four events (null collision, scattering, out of bounds, absorption) occurs at least 10 000 times; the extinction-0 cases leave the cube
as the contract does; and A_REF is tight (at least one case needs it)."""
import numpy as np
import pytest

from fast_twin_cases import (A_REF, CASES, EXTINCTION_0_SEEDS, PASSES, MAX_FRAGILE_CASE, MAX_FRAGILE_OVERALL, MIN_EVENTS_PER_CODE, CaseStats, case_id, drawn,
                             renderer, reset_frame, frame_of, hold_pass)
from test_gpu_fuzz import oracle_only

_DONE = {}


def run_case(oracle, key):
    """the case's PASSES passes on the oracle, each held to the twin; computed once"""
    if key in _DONE:
        return _DONE[key]
    d = drawn(key)
    osc = oracle.OracleScene(d["vol"], d["filt"], tf=d["tf"], env=d["env"])
    o = oracle.OracleRenderer("mcm", osc, d["w"], d["h"])
    stats = CaseStats(key)
    with oracle_only() as ctx:
        r = renderer(ctx, None, d)
        r.reset()
        o.reset(reset_frame(oracle, d))
        for _ in range(PASSES):
            r.render()
            fr = frame_of(oracle, d, r._u)
            assert fr.steps == d["steps"] and fr.blur == 0.0
            before = [s.copy() for s in o.state]
            o.integrate(fr)
            hold_pass(oracle, osc, fr, before, o.state, A_REF, stats)
        r.destroy()
    stats.extinction = d["extinction"]
    stats.left_cube = bool((o.state[3].reshape(-1, 4)[:, 3] == PASSES * d["steps"]).all())
    print(stats.line("contract oracle vs twin,"))
    _DONE[key] = stats
    return stats


@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_contract_oracle_agrees_with_the_twin(oracle, key):
    s = run_case(oracle, key)
    assert s.bad == 0, (s.line("contract oracle vs twin,"), s.first_bad)
    assert s.fragile_share <= MAX_FRAGILE_CASE, s.line("contract oracle vs twin,")
    if s.extinction == 0.0:                              # -log(u) * (1/0) = +inf: every event leaves the cube and ends a path, in both
        assert s.left_cube and s.codes[2] == s.pixel_events


def test_conditions_over_all_cases(oracle):
    all_ = [run_case(oracle, key) for key in CASES]
    events = sum(s.pixel_events for s in all_); fragile = sum(s.fragile for s in all_)
    codes = np.sum([s.codes for s in all_], axis=0)
    needed = max(s.needed for s in all_)
    print("contract oracle vs twin, all cases: %d pixel-events, %d fragile (%.4f %%), worst case %.3f %%, events null/scatter/out/absorb %s, A_ref %g"
          % (events, fragile, 100.0 * fragile / events, 100 * max(s.fragile_share for s in all_), list(codes), needed))
    assert sum(s.bad for s in all_) == 0
    assert fragile <= MAX_FRAGILE_OVERALL * events
    assert (codes >= MIN_EVENTS_PER_CODE).all(), list(codes)
    assert tuple(s.key[1] for s in all_ if s.key[0] == "seed" and s.extinction == 0.0) == EXTINCTION_0_SEEDS
    assert needed == A_REF, "A_REF is stated as %g, the cases need %g" % (A_REF, needed)
