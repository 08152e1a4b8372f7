// vpt_buffers.h — the one place that calls the allocator: move-only owners of device memory (DevBuf<T>) and of pinned host memory
// (PinnedBuf<T>).  Host only, nothing of the project's: tests/test_buffers.py builds it with a host compiler against counting stubs.
// No pooling, no caching: alloc is one hipMalloc / hipHostMalloc, reset and the destructor one hipFree / hipHostFree.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

struct DeviceMemory {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { (void)hipFree(p); }
};
struct PinnedMemory {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { (void)hipHostFree(p); }
};

template <typename T, typename Memory = DeviceMemory>
class DevBuf {
    T *p_ = nullptr;
    size_t count_ = 0;
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), count_(o.count_) { o.p_ = nullptr; o.count_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; count_ = o.count_; o.p_ = nullptr; o.count_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // frees what it holds, then allocates `count` elements; on failure the buffer is empty.  The caller has made sure that the device
    // no longer uses the old memory (reserve does that itself)
    hipError_t alloc(size_t count) {
        reset();
        void *p = nullptr;
        hipError_t e = Memory::get(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = (T *)p; count_ = count;
        return hipSuccess;
    }
    // the one grow rule: enough capacity is a compare and nothing else; otherwise what stream `s` still does with the old memory is
    // waited for, then it is freed and the larger one allocated (the contents are not carried over)
    hipError_t reserve(size_t count, hipStream_t s) {
        if (count <= count_) return hipSuccess;
        if (p_) { hipError_t e = hipStreamSynchronize(s); if (e != hipSuccess) return e; }
        return alloc(count);
    }
    void reset() {
        if (p_) Memory::put(p_);
        p_ = nullptr; count_ = 0;
    }
    size_t capacity() const { return count_; }     // in elements
    T *get() const { return p_; }
    operator T *() const { return p_; }
};
template <typename T> using PinnedBuf = DevBuf<T, PinnedMemory>;
