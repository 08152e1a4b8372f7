"""CPU: what a renderer's passes remember about the tile classes (vpt_amd/csrc/vpt_pass_state.h: Destinations, MarcherTrack, MissState),
compiled with the host compiler alone into a stand-alone program.  The set of destinations; every life of MCM's MISS-tile state of up to
DEPTH events, executed as vpt_mcm.hip executes them, with the invariants the settled forms of the MISS pass rest on checked after every
step; the 2^24 bound of the float sample count; lives that mirror tests/test_gpu_mcm_settled.py; the marchers' pass tracking.  The program
runs a second time under the address and undefined-behaviour sanitizers where the host compiler links them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vpt_amd", "csrc")
DEPTH = 5                 # 34 events (a pass that probes: three outcomes): 34^5 lives, a few seconds
DEPTH_SANITIZED = 4

PROGRAM = r"""
#include "vpt_pass_state.h"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

static long long failures = 0, steps_walked = 0, plans_settled = 0, plans_packed = 0, plans_probed = 0;
static const char *first_failure = "-";
#define CHECK(cond, name) do { if (!(cond) && !failures++) first_failure = name; } while (0)

static char memory[4096];
static const void *const A = memory, *const B = memory + 64;
static const uint64_t LIMIT = 1ull << 24;

// ---- MissState: a state and what the walk knows about its life from the outside ----
struct Life {
    MissState s;
    int option = 2, settle = 0, probes = 0;
    bool env_changed = false;
    uint64_t events = 0, settled = 0;
};
static void catch_up(Life &l) { if (l.s.owes()) l.s.materialized(); }               // mcm_catch_up
static void probe(Life &l, int outcome) {                                           // 0: final, 1: not yet, 2: no pixel to read
    l.s.probed(outcome != 2, outcome != 2, outcome == 0);
    l.probes++;
    if (outcome == 0) l.settle = 1;
    else if (outcome == 2 || l.probes >= 4) l.settle = 2;
}
// a pass over the tile classes as launch_mcm_classes executes it; returns whether the plan asked for a probe
static bool class_pass(Life &l, bool fuse, uint32_t steps, const void *dest, bool table, int n_miss, int outcome, bool fast = false,
                       bool plain_kernel = true, bool capturing = false, bool env_usable = true) {
    const MissPass p = { fuse, steps, plain_kernel, n_miss, capturing, env_usable, table, dest };
    MissPlan plan = l.s.plan(p);
    const bool probed = plan.probe_first;
    if (probed) {
        plans_probed++;
        CHECK(l.settle == 0 && l.s.pending() == 0, "a probe only while nothing is known and nothing is pending");
        probe(l, outcome);
        plan = l.s.plan(p, true);
        CHECK(!plan.probe_first, "one probe a pass");
    }
    const bool owed = l.s.owes(), fresh = l.s.words_fresh(), known = l.s.has_destination(dest);
    if (plan.form == MISS_PLAIN) CHECK(plan.catch_up_first == owed && !plan.materialize_first, "I2 PLAIN catches up while anything is owed");
    if (plan.form == MISS_SETTLED) CHECK(plan.materialize_first == fresh && !plan.catch_up_first, "I3 SETTLED materializes while the words are fresh");
    if (plan.form == MISS_PACKED) CHECK(!plan.materialize_first && !plan.catch_up_first, "PACKED runs on what is owed");
    if (plan.form != MISS_PLAIN) {
        CHECK(l.settle == 1 && !l.env_changed && l.events >= 1 && steps >= 1 && l.events + steps < LIMIT, "I4 the settled forms' conditions");
        CHECK(!fuse || (!table && known), "I4 a fused settled pass: no table, a known destination");
        CHECK(l.option != 0 && n_miss > 0 && plain_kernel && !capturing && env_usable, "the settled forms: the option, MISS tiles, the plain kernel, no capture");
        CHECK((plan.form == MISS_PACKED) == (l.option == 2), "I5 PACKED with option 2, and only then");
        (plan.form == MISS_PACKED ? plans_packed : plans_settled)++;
    }
    if (plan.materialize_first) { l.s.materialized(); CHECK(!l.s.owes() && !l.s.stale(), "I7"); }
    if (plan.catch_up_first) catch_up(l);
    CHECK(plan.form != MISS_PLAIN || !l.s.owes(), "nothing owed under a PLAIN pass");
    CHECK(plan.form != MISS_SETTLED || !l.s.words_fresh(), "no fresh words under a SETTLED pass");
    l.s.class_pass_done(plan.form, steps, fast, n_miss);
    l.s.events_run(steps);
    l.events += steps;
    if (plan.form != MISS_PLAIN) l.settled++;
    return probed;
}
static const int EVENTS = 34;
static bool step(Life &l, int e, int outcome) {
    switch (e) {
        case 0: case 1: l.s.reset(e == 1); l.settle = e; l.probes = 0; l.env_changed = false; l.events = 0; return false;
        case 2: l.s.geometry_rebuilt(); CHECK(!l.s.owes() && !l.s.stale() && !l.s.has_destination(A) && !l.s.has_destination(B), "a rebuild"); return false;
        case 3: catch_up(l); l.s.environment_changed(); l.env_changed = true; return false;        // mcm_environment_changed
        case 4: case 5: case 6: {
            const int v = e - 4;
            if (l.s.option_wants_catch_up(v)) catch_up(l);
            l.s.set_option(v); l.option = v;
            CHECK(v == 2 || !l.s.words_fresh(), "fresh words only under option 2");
            CHECK(v != 0 || !l.s.owes(), "nothing owed once the option is off");
            return false;
        }
        case 7: case 8: catch_up(l); l.s.bucket_done(e == 8, 5); l.s.events_run(8 * 3); l.events += 8 * 3; CHECK(l.s.stale_fast() == (e == 8), "bucket"); return false;   // mcm_bucket
        case 9: l.s.materialized(); l.s.events_run(8 * 2); l.events += 8 * 2; return false;           // mcm_multi: a whole-image sequence
        case 10: l.s.materialized(); CHECK(!l.s.owes() && !l.s.stale() && l.s.pending() == 0 && !l.s.words_fresh(), "I7"); return false;
        case 11: case 12: case 13: probe(l, e - 11); return false;
        default: break;
    }
    e -= 14;                                          // 4 passes that are not fused, 16 that are
    if (e < 4) return class_pass(l, false, (e & 1) ? 8 : 1, A, false, (e & 2) ? 5 : 0, outcome);
    e -= 4;
    return class_pass(l, true, (e & 1) ? 8 : 1, (e & 2) ? B : A, (e & 4) != 0, (e & 8) ? 5 : 0, outcome);
}
static void invariants(const Life &l) {
    CHECK(!l.s.words_fresh() || l.s.stale(), "I1 fresh words imply stale");
    CHECK(l.s.pending() == 0 || l.s.stale(), "I1 pending events imply stale");
    CHECK(l.s.owes() == (l.s.pending() > 0 || l.s.words_fresh()), "owes");
    CHECK(l.s.events() == l.events, "I6 the events are the steps of every pass since the reset");
    CHECK(l.s.settled_passes() == l.settled, "I8 one settled pass per SETTLED or PACKED pass");
    CHECK(l.s.pending() <= l.s.events(), "pending events are events");
}
static void walk(const Life &l, int depth) {
    if (depth == 0) return;
    for (int e = 0; e < EVENTS; e++)
        for (int outcome = 0; outcome < 3; outcome++) {
            Life n = l;
            const bool probed = step(n, e, outcome);
            invariants(n);
            steps_walked++;
            walk(n, depth - 1);
            if (!probed) break;                       // the outcome was not asked for: the three lives are one
        }
}
static int form_at(uint64_t events, uint32_t steps) {
    Life l;
    l.s.reset(true); l.settle = 1;
    l.s.events_run(events); l.events = events;
    const MissPass p = { false, steps, true, 5, false, true, false, A };
    return (int)l.s.plan(p).form;
}
static long settled_after(Life &l, int passes, int outcome = 0) {
    for (int i = 0; i < passes; i++) class_pass(l, true, 5, A, false, 7, outcome);
    invariants(l);
    return (long)l.s.settled_passes();
}

// ---- MarcherTrack ----
static float M1[16], M2[16];
struct Marcher {
    MarcherTrack t; int kind; bool opaque;
    bool fused(const float *m, const void *dest, float mix = 0.5f, bool enabled = true, bool capturing = false) {
        const bool lists = t.pass(kind, m, true, mix, enabled, capturing, opaque, dest);
        if (lists) t.use_lists(true);
        const bool now = t.list_now();
        t.use_lists(false);
        return now;
    }
};
static Marcher marcher(int kind, bool opaque = true) { Marcher m; m.kind = kind; m.opaque = opaque; m.t.reset(); return m; }
static void bits(const char *name, std::initializer_list<bool> b) {
    std::printf("%s ", name);
    for (bool x : b) std::printf("%d", x ? 1 : 0);
    std::printf("\n");
}

int main(int argc, char **argv) {
    const int depth = argc > 1 ? std::atoi(argv[1]) : 3;
    {
        Destinations d;
        bool ok = d.size() == 0 && !d.has(A);
        d.add(A); d.add(B); d.add(A);
        ok = ok && d.size() == 2 && d.has(A) && d.has(B);
        d.remove(A); ok = ok && d.size() == 1 && !d.has(A) && d.has(B);
        d.remove(A); ok = ok && d.size() == 1;
        d.clear(); ok = ok && d.size() == 0 && !d.has(B);
        std::printf("dest_basic %d\n", ok);
        for (int i = 0; i < VPT_COMPLETE_DESTS + 1; i++) d.add(memory + 8 * i);
        ok = d.size() == VPT_COMPLETE_DESTS && !d.has(memory + 8 * VPT_COMPLETE_DESTS);
        for (int i = 0; i < VPT_COMPLETE_DESTS; i++) ok = ok && d.has(memory + 8 * i);
        d.add(memory); ok = ok && d.size() == VPT_COMPLETE_DESTS;
        std::printf("dest_full %d\n", ok);
        d.remove_range(memory + 8 * 3, 8 * 4);         // [3, 7)
        ok = d.size() == VPT_COMPLETE_DESTS - 4;
        for (int i = 0; i < VPT_COMPLETE_DESTS; i++) ok = ok && d.has(memory + 8 * i) == (i < 3 || i >= 7);
        d.remove_range(memory + 8 * 7 + 1, 7);         // between two entries: nothing
        ok = ok && d.size() == VPT_COMPLETE_DESTS - 4 && d.has(memory + 8 * 7) && d.has(memory + 8 * 8);
        d.remove_range(memory, sizeof(memory));
        std::printf("dest_range %d\n", ok && d.size() == 0);
    }
    {
        walk(Life(), depth);
        std::printf("walk %d %lld %lld %lld %lld %lld %s\n", depth, steps_walked, failures, plans_settled, plans_packed, plans_probed, first_failure);
    }
    std::printf("limit %d %d %d %d\n", form_at(LIMIT - 8 - 1, 8), form_at(LIMIT - 8, 8), form_at(LIMIT - 1 - 1, 1), form_at(LIMIT - 1, 1));
    {
        const MissPass base = { false, 8, true, 5, false, true, false, A };
        int forced = 0;
        for (int k = 0; k < 5; k++) {
            Life l; l.s.reset(true); l.s.events_run(8);
            MissPass p = base;
            if (k == 0) p.plain_kernel = false; else if (k == 1) p.capturing = true; else if (k == 2) p.env_usable = false; else if (k == 3) p.n_miss = 0; else p.steps = 0;
            forced += l.s.plan(p).form == MISS_PLAIN;
        }
        Life l; l.s.reset(true); l.s.events_run(8);
        std::printf("plain_forced %d %d\n", forced, (int)l.s.plan(base).form);
    }
    {
        Life a; step(a, 1, 0);                                              // a settling environment
        std::printf("life_plain %ld\n", settled_after(a, 6));
        Life b; step(b, 0, 0);                                              // settled by the probe in front of the second pass
        const long first = settled_after(b, 3);
        step(b, 10, 0);                                                     // a read-back
        std::printf("life_read_back %ld %ld\n", first, settled_after(b, 3));
        Life c; step(c, 1, 0);
        const long before = settled_after(c, 2);
        step(c, 3, 0);
        const long after = settled_after(c, 4);
        step(c, 1, 0);
        std::printf("life_environment %ld %ld %ld\n", before, after, settled_after(c, 2));
        Life d; step(d, 0, 0);                                              // never final: four probes, then given up
        const long never = settled_after(d, 8, 1);
        std::printf("life_never_final %ld %d\n", never, d.probes);
        std::printf("life_failures %lld %s\n", failures, first_failure);
    }
    {
        for (int i = 0; i < 16; i++) { M1[i] = (float)i; M2[i] = (float)i; }
        M2[5] = -1.0f;
        Marcher m = marcher(VPT_RENDERER_MIP);
        const bool p1 = m.fused(M1, A), known = m.t.has_destination(A), p2 = m.fused(M1, A), p3 = m.fused(M1, A);
        bits("marcher_basic", { p1, known, p2, p3 });
        Marcher a = m; bits("marcher_matrix", { a.fused(M2, A), a.fused(M1, A), (a.t.reset(), a.fused(M1, A)), a.fused(M1, A) });
        Marcher b = m; b.t.environment_changed(); bits("marcher_environment", { b.fused(M1, A), b.fused(M1, A), (b.t.reset(), b.fused(M1, A)), b.fused(M1, A) });
        Marcher c = m; c.t.geometry_rebuilt(); bits("marcher_rebuild", { c.fused(M1, A), c.fused(M1, A), c.fused(M1, A), (c.t.reset(), c.fused(M1, A)), c.fused(M1, A) });
        Marcher d = m; bits("marcher_destinations", { d.fused(M1, B), d.fused(M1, B), d.fused(M1, A), (d.t.forget_destinations(A, 1), d.fused(M1, A)), d.fused(M1, A),
                                                      (d.t.forget_destinations(memory, 128), d.fused(M1, B)), d.fused(M1, A), d.fused(M1, B) });
        Marcher e = m; bits("marcher_off", { e.fused(M1, A, 0.5f, false), e.fused(M1, A, 0.5f, true, true), e.fused(M1, A) });
        Marcher g = marcher(VPT_RENDERER_EAM);
        const bool generate = g.t.pass(VPT_RENDERER_EAM, M1, false, 0.0f, true, false, true, A);
        bits("marcher_generate", { generate, g.t.has_destination(A), g.fused(M1, A), g.fused(M1, A) });
        Marcher r = marcher(VPT_RENDERER_ISO); r.t.replayed(VPT_RENDERER_ISO, M1, 0.5f, A);
        bits("marcher_replayed", { r.t.list_now(), r.t.has_destination(A), r.fused(M1, A) });
        auto second = [](int kind, float mix, bool opaque) { Marcher x = marcher(kind, opaque); x.fused(M1, A, mix); return x.fused(M1, A, 0.25f); };
        bits("marcher_fixed_points", { second(VPT_RENDERER_DEPTH, 1.0f, false), second(VPT_RENDERER_DEPTH, 0.5f, true), second(VPT_RENDERER_MCS, 1.0f, true),
                                       second(VPT_RENDERER_MCS, 1.0f, false), second(VPT_RENDERER_MCS, 0.5f, true), second(VPT_RENDERER_ISO, 0.5f, false),
                                       second(VPT_RENDERER_MCM, 1.0f, true), second(VPT_RENDERER_LAO, 1.0f, true) });
    }
    return 0;
}
"""


def _compiler():
    return next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)


def _run(tmp, name, depth, flags=()):
    exe = str(tmp / name)
    subprocess.run([_compiler(), "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I", CSRC, "-x", "c++", "-", "-o", exe], input=PROGRAM.encode(), check=True)
    rows = {}
    for line in subprocess.check_output([exe, str(depth)]).decode().splitlines():
        name, *values = line.split(" ", 1)
        rows[name] = values[0] if values else ""
    return rows


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    if _compiler() is None:
        pytest.skip("no host C++ compiler")
    return _run(tmp_path_factory.mktemp("pass_state"), "pass_state", DEPTH)


def _check(rows, depth):
    assert rows["dest_basic"] == "1" and rows["dest_full"] == "1" and rows["dest_range"] == "1"
    walked_depth, steps, failures, settled, packed, probed, first = rows["walk"].split(" ", 6)
    assert int(failures) == 0, first
    assert int(walked_depth) == depth and int(steps) >= sum(34 ** k for k in range(1, depth + 1))
    assert int(settled) > 0 and int(packed) > 0 and int(probed) > 0          # the walk reached every form
    # a settled form (PACKED = 1 under the default option) while events + steps < 2^24, PLAIN = 0 from there on
    assert rows["limit"] == "1 0 1 0"
    assert rows["plain_forced"] == "5 1"
    assert rows["life_plain"] == "5"
    assert rows["life_read_back"] == "2 5"
    assert rows["life_environment"] == "1 1 2"
    assert rows["life_never_final"] == "0 4"
    assert rows["life_failures"].split(" ", 1)[0] == "0", rows["life_failures"]


def test_the_set_of_destinations_and_every_life_of_the_miss_state(rows):
    _check(rows, DEPTH)


def test_the_marchers_ask_for_lists_only_where_the_skipped_tiles_are_in_place(rows):
    assert rows["marcher_basic"] == "0111"              # a whole-image pass makes its destination known; the second pass asks
    assert rows["marcher_matrix"] == "0001"             # another matrix: none until the reset, then one whole pass first
    assert rows["marcher_environment"] == "0001"
    assert rows["marcher_rebuild"] == "00001"           # zero-filled buffers are not a reset
    # B takes a whole pass first; A is still known; forgotten, it takes one again; a forgotten range holds both
    assert rows["marcher_destinations"] == "01101001"
    assert rows["marcher_off"] == "001"                 # classes off, a capture running
    assert rows["marcher_generate"] == "0001"           # a generate pass is no fused pass and writes no destination
    assert rows["marcher_replayed"] == "011"            # a replayed frame is a whole-image fused pass
    # Depth with mix 1; Depth with another; MCS with mix 1 under an opaque environment; not opaque; another mix; ISO always; MCM, LAO never
    assert rows["marcher_fixed_points"] == "10100100"


def test_the_header_is_host_only():
    text = open(os.path.join(CSRC, "vpt_pass_state.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<string.h>", '"../../include/vpt.h"'], includes       # (the C ABI: the renderer kinds, the integer types)
    assert re.search(r"^COMMON\s*:=.*\bvpt_pass_state\.h\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert '#include "vpt_pass_state.h"' in open(os.path.join(CSRC, "vpt_internal.h")).read()


def test_the_same_program_under_the_sanitizers(tmp_path):
    if _compiler() is None:
        pytest.skip("no host C++ compiler")
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    probe = subprocess.run([_compiler(), *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input=b"int main() { return 0; }", capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the host compiler links no sanitizer runtimes")
    _check(_run(tmp_path, "pass_state_sanitized", DEPTH_SANITIZED, flags), DEPTH_SANITIZED)
