"""CPU: the owners of device and pinned memory (vpt_amd/csrc/vpt_buffers.h), compiled with the host compiler alone against counting
stubs of hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipStreamSynchronize (nothing of ROCm is linked, only its header is read):
every scope ends with no live allocation, also one left early; a move hands the memory on and it is freed once; a failed allocation
leaves the buffer empty; reserve calls nothing while the capacity suffices and otherwise waits for the stream, frees, allocates — in that
order; reset may be repeated."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vpt_amd", "csrc")

PROGRAM = r"""
#include "vpt_buffers.h"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>

static std::set<void *> live_device, live_pinned;
static std::string trace;                 // the calls since the last clear: m(alloc) f(ree) M(alloc pinned) F(ree pinned) s(ynchronise)
static int fail_in = 0;                   // the n-th allocation from now fails (0: none)
static int bad_frees = 0;                 // frees of something not live (a double free among them)
static hipStream_t synced = nullptr;

static hipError_t get(std::set<void *> &live, void **p, size_t n, char c) {
    trace += c;
    if (fail_in && --fail_in == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(n ? n : 1);
    live.insert(*p);
    return hipSuccess;
}
static hipError_t put(std::set<void *> &live, void *p, char c) {
    trace += c;
    if (!live.erase(p)) { bad_frees++; return hipErrorInvalidValue; }
    std::free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMalloc(void **p, size_t n) { return get(live_device, p, n, 'm'); }
extern "C" hipError_t hipFree(void *p) { return put(live_device, p, 'f'); }
extern "C" hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return get(live_pinned, p, n, 'M'); }
extern "C" hipError_t hipHostFree(void *p) { return put(live_pinned, p, 'F'); }
extern "C" hipError_t hipStreamSynchronize(hipStream_t s) { trace += 's'; synced = s; return hipSuccess; }

static size_t live() { return live_device.size() + live_pinned.size(); }
static void report(const char *name, long a = 0, long b = 0, long c = 0, long d = 0) {
    std::printf("%s %s %zu %d %ld %ld %ld %ld\n", name, trace.empty() ? "-" : trace.c_str(), live(), bad_frees, a, b, c, d);
    trace.clear();
}
// three steps of which the third fails: the function is left through the error return, as HIP_TRY leaves one
static hipError_t left_early(size_t *live_inside) {
    DevBuf<float> a; PinnedBuf<int> b; DevBuf<double> c;
    hipError_t e;
    if ((e = a.alloc(100)) != hipSuccess) return e;
    if ((e = b.alloc(100)) != hipSuccess) return e;
    *live_inside = live();
    fail_in = 1;
    if ((e = c.alloc(100)) != hipSuccess) return e;
    return hipSuccess;
}
int main() {
    hipStream_t stream = (hipStream_t)(void *)&trace;       // any non-null handle: the stub only records it
    {
        size_t inside;
        { DevBuf<float> a; PinnedBuf<int> b; (void)a.alloc(10); (void)b.alloc(4); inside = live(); }
        report("scope", (long)inside);
    }
    {
        size_t inside = 0;
        hipError_t e = left_early(&inside);
        report("early", (long)inside, e == hipErrorOutOfMemory);
    }
    {
        bool ok;
        {
            DevBuf<int> a; (void)a.alloc(7);
            int *p = a.get();
            DevBuf<int> b(std::move(a));                      // move construction
            ok = a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 7;
            DevBuf<int> c; (void)c.alloc(3);
            c = std::move(b);                                 // move assignment: c's own memory is freed, b's handed on
            ok = ok && b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 7 && live() == 1;
        }
        report("move", ok);
    }
    {
        DevBuf<int> a; PinnedBuf<int> b;
        fail_in = 1; hipError_t ea = a.alloc(5);
        fail_in = 1; hipError_t eb = b.alloc(5);
        report("alloc_fails", ea == hipErrorOutOfMemory && eb == hipErrorOutOfMemory, a.get() == nullptr && b.get() == nullptr, (long)a.capacity(), (long)b.capacity());
        (void)a.alloc(5);
        fail_in = 1; ea = a.alloc(9);                         // what it held is gone too: empty, not stale
        report("alloc_fails_holding", ea == hipErrorOutOfMemory, a.get() == nullptr, (long)a.capacity());
    }
    {
        DevBuf<short> a; (void)a.alloc(8);
        short *p = a.get();
        trace.clear();
        hipError_t e1 = a.reserve(8, stream), e2 = a.reserve(3, stream), e3 = a.reserve(0, stream);
        report("reserve_enough", e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess, a.get() == p, (long)a.capacity());
        synced = nullptr;
        hipError_t e = a.reserve(16, stream);
        report("reserve_grows", e == hipSuccess, synced == stream, (long)a.capacity(), a.get() != nullptr);
        PinnedBuf<short> b; (void)b.reserve(4, stream);
        trace.clear();
        (void)b.reserve(5, stream);
        report("reserve_grows_pinned", (long)b.capacity());
    }
    report("after_reserve");
    {
        DevBuf<int> a; (void)a.alloc(2);
        trace.clear();
        a.reset(); a.reset();
        DevBuf<int> never; never.reset();
        report("reset_twice", a.get() == nullptr, (long)a.capacity());
    }
    report("end");
    return 0;
}
"""


def rocm_include():
    roots = [os.environ.get(k) for k in ("ROCM_PATH", "HIP_PATH")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    roots.append("/opt/rocm")
    for root in roots:
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    include = rocm_include()
    if include is None:
        pytest.skip("no ROCm headers")
    exe = str(tmp_path_factory.mktemp("buffers") / "buffers")
    # (no -Werror: the ROCm header marks results nodiscard and warns in places of its own)
    subprocess.run([cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I", CSRC, "-x", "c++", "-", "-o", exe], input=PROGRAM.encode(), check=True)
    out = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        name, trace, live, bad, *values = line.split()
        out[name] = ("" if trace == "-" else trace, int(live), int(bad), [int(v) for v in values])
    return out


def test_header_is_small_and_host_only():
    text = open(os.path.join(CSRC, "vpt_buffers.h")).read()
    assert len(text.splitlines()) < 100
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<stddef.h>"], includes


def test_nothing_is_live_after_any_scope_and_nothing_is_freed_twice(rows):
    inside_a_scope = {"reserve_enough": 1, "reserve_grows": 1, "reserve_grows_pinned": 2}      # reported while their buffers are held
    for name, (_, live, bad, _) in rows.items():
        assert live == inside_a_scope.get(name, 0), name
        assert bad == 0, name
    assert set(rows) == {"scope", "early", "move", "alloc_fails", "alloc_fails_holding", "reserve_enough", "reserve_grows", "reserve_grows_pinned",
                         "after_reserve", "reset_twice", "end"}


def test_a_scope_frees_what_it_allocated_each_from_its_own_allocator(rows):
    trace, _, _, (inside, *_) = rows["scope"]
    assert inside == 2
    assert sorted(trace) == sorted("mMfF"), trace


def test_a_scope_left_early_through_a_failing_step_frees_what_was_built(rows):
    trace, _, _, (inside, out_of_memory, *_) = rows["early"]
    assert inside == 2 and out_of_memory == 1
    assert trace[:3] == "mMm" and sorted(trace[3:]) == ["F", "f"], trace      # the failed third allocation holds nothing to free


def test_a_move_transfers_ownership_and_frees_once(rows):
    trace, _, _, (ok, *_) = rows["move"]
    assert ok == 1
    assert trace == "mmff", trace          # two allocations; c's own at the assignment, the moved one at the end of the scope — nothing for a and b


def test_a_failed_alloc_returns_the_error_and_leaves_the_buffer_empty(rows):
    trace, _, _, (errors, null, cap_device, cap_pinned) = rows["alloc_fails"]
    assert errors == 1 and null == 1 and cap_device == 0 and cap_pinned == 0
    assert trace == "mM", trace
    trace, _, _, (error, null, cap, _) = rows["alloc_fails_holding"]
    assert error == 1 and null == 1 and cap == 0
    assert trace == "mfm", trace


def test_reserve_with_enough_capacity_calls_nothing(rows):
    trace, _, _, (ok, same_pointer, cap, _) = rows["reserve_enough"]
    assert trace == ""
    assert ok == 1 and same_pointer == 1 and cap == 8


def test_reserve_that_grows_synchronises_then_frees_then_allocates(rows):
    trace, _, _, (ok, on_the_stream_given, cap, holds) = rows["reserve_grows"]
    assert trace == "sfm", trace
    assert ok == 1 and on_the_stream_given == 1 and cap == 16 and holds == 1
    trace, _, _, (cap, *_) = rows["reserve_grows_pinned"]
    assert trace == "sFM" and cap == 5, trace
    assert sorted(rows["after_reserve"][0]) == ["F", "f"]      # the two buffers of that scope


def test_reset_twice_frees_once(rows):
    trace, _, _, (null, cap, *_) = rows["reset_twice"]
    assert trace == "f", trace
    assert null == 1 and cap == 0
    assert rows["end"][0] == ""
