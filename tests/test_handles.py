"""CPU: the owners of HIP events and streams and the pool of timing event pairs (vpt_amd/csrc/vpt_handles.h), compiled with the host
compiler alone against counting stubs of hipEventCreateWithFlags / hipEventDestroy / hipStreamCreateWithFlags / hipStreamDestroy (nothing
of ROCm is linked, only its header is read): every scope ends with nothing live, also one left early; a move hands the handle on and it
is destroyed once; a failed create leaves the owner empty; reset may be repeated; the pool creates a pair only when it has none left,
keeps nothing of a failed attempt and reports the launches of the latest take.  And the source-level side of it: no other file of the
library creates or destroys an event or a stream, the objects hold theirs through the owner types."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from test_buffers import rocm_include

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vpt_amd", "csrc")

PROGRAM = r"""
#include "vpt_handles.h"
#include <cstdio>
#include <set>
#include <string>
#include <utility>

static std::set<void *> live_events, live_streams;
static std::string trace;                 // the calls since the last clear: e(vent created) E(vent destroyed) s(tream created) S(tream destroyed)
static int fail_in = 0;                   // the n-th creation from now fails (0: none)
static int bad_destroys = 0;              // destroys of something not live (a second destroy among them)
static unsigned last_flags = 0;

template <typename T> static hipError_t make(std::set<void *> &live, T *h, unsigned flags, char c) {
    trace += c; last_flags = flags;
    if (fail_in && --fail_in == 0) { *h = (T)(void *)&fail_in; return hipErrorOutOfMemory; }    // (a failing create may scribble on its output)
    void *p = new char;
    live.insert(p); *h = (T)p;
    return hipSuccess;
}
static hipError_t drop(std::set<void *> &live, void *p, char c) {
    trace += c;
    if (!live.erase(p)) { bad_destroys++; return hipErrorInvalidValue; }
    delete (char *)p;
    return hipSuccess;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) { return make(live_events, e, flags, 'e'); }
extern "C" hipError_t hipEventDestroy(hipEvent_t e) { return drop(live_events, (void *)e, 'E'); }
extern "C" hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) { return make(live_streams, s, flags, 's'); }
extern "C" hipError_t hipStreamDestroy(hipStream_t s) { return drop(live_streams, (void *)s, 'S'); }

static size_t live() { return live_events.size() + live_streams.size(); }
static long used(const EventPairs &pool) {                 // the pairs taken since the last rewind
    long n = 0;
    for (const EventPairs::Pair *p = pool.first(); p; p = pool.after(p)) n++;
    return n;
}
static void report(const char *name, long a = 0, long b = 0, long c = 0, long d = 0) {
    std::printf("%s %s %zu %d %ld %ld %ld %ld\n", name, trace.empty() ? "-" : trace.c_str(), live(), bad_destroys, a, b, c, d);
    trace.clear();
}
// three steps of which the third fails: the function is left through the error return, as HIP_TRY leaves one
static hipError_t left_early(size_t *live_inside) {
    Stream a; Event b, c;
    hipError_t e;
    if ((e = a.create()) != hipSuccess) return e;
    if ((e = b.create(hipEventDisableTiming)) != hipSuccess) return e;
    *live_inside = live();
    fail_in = 1;
    if ((e = c.create(hipEventDisableTiming)) != hipSuccess) return e;
    return hipSuccess;
}
int main() {
    {
        size_t inside; bool flags;
        {
            Event a; Stream b;
            bool empty = a.get() == nullptr && b.get() == nullptr && !a && !b;
            (void)a.create(hipEventDisableTiming); flags = empty && last_flags == hipEventDisableTiming;
            (void)b.create(); flags = flags && last_flags == hipStreamNonBlocking;
            hipEvent_t raw = a; hipStream_t raw_stream = b;       // the implicit conversions calls of the runtime rely on
            flags = flags && raw == a.get() && raw != nullptr && raw_stream == b.get() && raw_stream != nullptr;
            inside = live();
        }
        report("scope", (long)inside, flags);
    }
    {
        size_t inside = 0;
        hipError_t e = left_early(&inside);
        report("early", (long)inside, e == hipErrorOutOfMemory);
    }
    {
        bool ok;
        {
            Event a; (void)a.create();
            hipEvent_t h = a.get();
            Event b(std::move(a));                            // move construction
            ok = a.get() == nullptr && b.get() == h;
            Event c; (void)c.create();
            c = std::move(b);                                 // move assignment: c's own event is destroyed, b's handed on
            ok = ok && b.get() == nullptr && c.get() == h && live() == 1;
            Stream s; (void)s.create();
            Stream t(std::move(s));
            ok = ok && s.get() == nullptr && t.get() != nullptr && live() == 2;
        }
        report("move", ok);
    }
    {
        Event a; Stream b;
        fail_in = 1; hipError_t ea = a.create();
        fail_in = 1; hipError_t eb = b.create();
        report("create_fails", ea == hipErrorOutOfMemory && eb == hipErrorOutOfMemory, a.get() == nullptr && b.get() == nullptr);
        (void)a.create();
        fail_in = 1; ea = a.create();                         // what it held is gone too: empty, not stale
        report("create_fails_holding", ea == hipErrorOutOfMemory, a.get() == nullptr);
    }
    {
        Event a; (void)a.create();
        Stream b; (void)b.create();
        trace.clear();
        a.reset(); a.reset(); b.reset(); b.reset();
        Event never; never.reset();
        Stream never_either; never_either.reset();
        report("reset_twice", a.get() == nullptr && b.get() == nullptr);
    }
    {
        EventPairs pool;
        EventPairs::Pair *p0 = pool.take(1), *p1 = pool.take(7);
        bool ok = p0 && p1 && p0 != p1 && p0->t0.get() && p0->t1.get() && p0->t0.get() != p0->t1.get() && last_flags == hipEventDefault;
        ok = ok && pool.first() == p0 && pool.after(p0) == p1 && pool.after(p1) == nullptr;
        report("pool_take", ok, (long)(live_events.size() / 2), used(pool), (long)p1->launches);
        pool.rewind();
        bool none = pool.first() == nullptr;
        EventPairs::Pair *again = pool.take(3);
        ok = none && again == p0 && pool.first() == p0 && pool.after(p0) == nullptr;
        report("pool_reuse", ok, (long)(live_events.size() / 2), used(pool), (long)again->launches);
        (void)pool.take(1);                                   // p1 again: the pool is exhausted from here on
        trace.clear();
        fail_in = 2;                                          // the second event of the new pair
        EventPairs::Pair *failed = pool.take(1);
        report("pool_second_fails", failed == nullptr, (long)(live_events.size() / 2), used(pool), pool.after(p1) == nullptr);
        fail_in = 1;                                          // the first event of the new pair
        failed = pool.take(1);
        report("pool_first_fails", failed == nullptr, (long)(live_events.size() / 2), used(pool));
        EventPairs::Pair *p2 = pool.take(5);
        ok = p2 && p2 != p0 && p2 != p1 && pool.after(p1) == p2 && pool.after(p2) == nullptr;
        report("pool_recovers", ok, (long)(live_events.size() / 2), used(pool), (long)p2->launches);
    }
    report("end");
    return 0;
}
"""


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    include = rocm_include()
    if include is None:
        pytest.skip("no ROCm headers")
    exe = str(tmp_path_factory.mktemp("handles") / "handles")
    # (no -Werror: the ROCm header marks results nodiscard and warns in places of its own)
    subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I", CSRC, "-x", "c++", "-", "-o", exe], input=PROGRAM.encode(), check=True)
    out = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        name, trace, live, bad, *values = line.split()
        out[name] = ("" if trace == "-" else trace, int(live), int(bad), [int(v) for v in values])
    return out


def test_header_is_small_and_host_only():
    text = open(os.path.join(CSRC, "vpt_handles.h")).read()
    assert len(text.splitlines()) < 100
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>"], includes


def test_nothing_is_live_after_any_scope_and_nothing_is_destroyed_twice(rows):
    # reported while the pool is alive: the events of its pairs
    inside_a_scope = {"pool_take": 4, "pool_reuse": 4, "pool_second_fails": 4, "pool_first_fails": 4, "pool_recovers": 6}
    for name, (_, live, bad, _) in rows.items():
        assert live == inside_a_scope.get(name, 0), name
        assert bad == 0, name
    assert set(rows) == {"scope", "early", "move", "create_fails", "create_fails_holding", "reset_twice", "pool_take", "pool_reuse",
                         "pool_second_fails", "pool_first_fails", "pool_recovers", "end"}


def test_a_scope_destroys_what_it_created_with_the_flags_asked_for(rows):
    trace, _, _, (inside, flags, *_) = rows["scope"]
    assert inside == 2 and flags == 1          # a stream is non-blocking unless told otherwise
    assert trace[:2] == "es" and sorted(trace[2:]) == ["E", "S"], trace


def test_a_scope_left_early_through_a_failing_third_creation_destroys_what_was_built(rows):
    trace, _, _, (inside, out_of_memory, *_) = rows["early"]
    assert inside == 2 and out_of_memory == 1
    assert trace[:3] == "see" and sorted(trace[3:]) == ["E", "S"], trace      # the failed third creation holds nothing to destroy


def test_a_move_hands_the_handle_on_and_it_is_destroyed_once(rows):
    trace, _, _, (ok, *_) = rows["move"]
    assert ok == 1
    assert trace[:4] == "eeEs" and sorted(trace[4:]) == ["E", "S"], trace     # c's own event at the assignment, the moved ones at the end


def test_a_failed_create_returns_the_error_and_leaves_the_owner_empty(rows):
    trace, _, _, (errors, null, *_) = rows["create_fails"]
    assert errors == 1 and null == 1
    assert trace == "es", trace
    trace, _, _, (error, null, *_) = rows["create_fails_holding"]
    assert error == 1 and null == 1
    assert trace == "eEe", trace


def test_reset_twice_destroys_once_and_an_empty_owner_calls_nothing(rows):
    trace, _, _, (null, *_) = rows["reset_twice"]
    assert trace == "ES", trace
    assert null == 1


def test_the_pool_creates_a_pair_only_when_none_is_left(rows):
    trace, _, _, (ok, size, used, launches) = rows["pool_take"]
    assert trace == "eeee" and (ok, size, used, launches) == (1, 2, 2, 7), trace
    trace, _, _, (ok, size, used, launches) = rows["pool_reuse"]
    assert trace == "", trace                                      # a take after a rewind creates nothing
    assert (ok, size, used) == (1, 2, 1)
    assert launches == 3                                           # of a reused pair: the value of the latest take


def test_a_take_that_cannot_create_leaves_the_pool_as_it_was(rows):
    trace, _, _, (null, size, used, last_unchanged) = rows["pool_second_fails"]
    assert trace == "eeE", trace                                   # the first event of the attempt is destroyed again
    assert (null, size, used, last_unchanged) == (1, 2, 2, 1)
    trace, _, _, (null, size, used, _) = rows["pool_first_fails"]
    assert trace == "e", trace
    assert (null, size, used) == (1, 2, 2)
    trace, _, _, (ok, size, used, launches) = rows["pool_recovers"]
    assert trace == "ee" and (ok, size, used, launches) == (1, 3, 3, 5), trace
    assert sorted(rows["end"][0]) == ["E"] * 6                     # the pool's three pairs go with it


CALLS = re.compile(r"hipEventCreate|hipEventDestroy|hipStreamCreate|hipStreamDestroy")


def test_only_the_header_creates_and_destroys_events_and_streams():
    files = [p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and os.path.splitext(p)[1] in (".h", ".hip", "") and
             os.path.basename(p) != "vpt_handles.h"]
    assert len(files) > 20
    found = {os.path.basename(p): sorted(set(CALLS.findall(open(p, errors="replace").read()))) for p in files}
    assert {name: calls for name, calls in found.items() if calls} == {}
    assert re.search(r"^COMMON\s*:=.*\bvpt_handles\.h\b", open(os.path.join(CSRC, "Makefile")).read(), re.M)
    assert '#include "vpt_handles.h"' in open(os.path.join(CSRC, "vpt_internal.h")).read()


def test_the_objects_hold_their_events_and_streams_through_the_owner_types():
    internal = open(os.path.join(CSRC, "vpt_internal.h")).read()
    post = open(os.path.join(CSRC, "vpt_post.hip")).read()
    core = open(os.path.join(CSRC, "vpt_core.hip")).read()
    for text, member in [(internal, r"Event staged\[2\]"), (internal, r"Stream side\[VPT_MAX_SPLIT - 1\]"), (internal, r"Event ev_fork\b"),
                         (internal, r"\bev_join\[VPT_MAX_SPLIT - 1\]"), (internal, r"const Event \*stop_events\b"), (internal, r"Stream own\b"),
                         (internal, r"EventPairs timing\b"), (internal, r"\bside_timing\b"),
                         (post, r"Stream comm_stream\b"), (post, r"Event rendered\[2\]\[VPT_MAX_SPLIT\]"), (post, r"\bgathered\[2\]"),
                         (core, r"Stream tried\[8\]"), (core, r"create_overlapping_stream\(Stream \*out")]:
        assert re.search(member, text), member
    for text, gone in [(internal, r"hipEvent_t\s*\*?\s*(staged|ev_fork|ev_join|stop_events)"), (internal, r"hipStream_t side\b"), (internal, r"owns_stream"),
                       (internal, r"\bevents_used\b|\bevent_launches\b|\bside_events\b"), (post, r"hipEvent_t (rendered|gathered)"),
                       (post, r"hipStream_t comm_stream"), (core, r"destroy_split_streams"), (core, r"hipEvent_t e0")]:
        assert not re.search(gone, text), gone
