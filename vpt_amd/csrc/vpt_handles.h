// vpt_handles.h — the one place that creates and destroys HIP events and streams: move-only owners of one event (Event) and of one stream
// (Stream), and the pool of timing event pairs behind vpt_renderer_set_profiling (EventPairs).  Host only, nothing of the project's:
// tests/test_handles.py builds it with a host compiler against counting stubs.  No pooling of handles, no adopt / release: a handle
// somebody else owns stays a plain hipStream_t beside the owner (vpt_context).
#pragma once
#include <hip/hip_runtime_api.h>

struct EventHandle {
    typedef hipEvent_t type;
    static const unsigned default_flags = hipEventDefault;
    static hipError_t make(type *h, unsigned flags) { return hipEventCreateWithFlags(h, flags); }
    static void drop(type h) { (void)hipEventDestroy(h); }
};
struct StreamHandle {
    typedef hipStream_t type;
    static const unsigned default_flags = hipStreamNonBlocking;
    static hipError_t make(type *h, unsigned flags) { return hipStreamCreateWithFlags(h, flags); }
    static void drop(type h) { (void)hipStreamDestroy(h); }
};

template <typename Kind>
class Handle {
    typename Kind::type h_ = nullptr;
public:
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Handle() { reset(); }
    // destroys what it holds, then creates; on failure the owner is empty.  The caller has made sure that nothing is in flight on the old handle
    hipError_t create(unsigned flags = Kind::default_flags) {
        reset();
        hipError_t e = Kind::make(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    void reset() {
        if (h_) Kind::drop(h_);
        h_ = nullptr;
    }
    typename Kind::type get() const { return h_; }
    operator typename Kind::type() const { return h_; }
};
typedef Handle<EventHandle> Event;
typedef Handle<StreamHandle> Stream;

// Timing event pairs, handed out in order and kept for the next round: take() creates a pair only when every pair made so far is in use,
// rewind() makes them all available again.  A pair stays where it is while the pool lives (a list, not an array that moves when it grows).
class EventPairs {
public:
    struct Pair { Event t0, t1; uint32_t launches = 0; Pair *next = nullptr; };   // launches: kernel launches the pair brackets
    EventPairs() = default;
    EventPairs(const EventPairs &) = delete;
    EventPairs &operator=(const EventPairs &) = delete;
    ~EventPairs() { while (head_) { Pair *p = head_; head_ = p->next; delete p; } }
    // the next pair, or null when one had to be created and could not be: then the pool is as it was and nothing of the attempt is live
    Pair *take(uint32_t launches) {
        Pair *&slot = last_ ? last_->next : head_;
        if (!slot) {
            Pair *p = new Pair;
            if (p->t0.create() != hipSuccess || p->t1.create() != hipSuccess) { delete p; return nullptr; }
            slot = p;
        }
        last_ = slot;
        last_->launches = launches;
        return last_;
    }
    void rewind() { last_ = nullptr; }
    // the pairs taken since the last rewind, in order: for (p = first(); p; p = after(p))
    const Pair *first() const { return last_ ? head_ : nullptr; }
    const Pair *after(const Pair *p) const { return p == last_ ? nullptr : p->next; }
private:
    Pair *head_ = nullptr, *last_ = nullptr;   // every pair made so far; the pair taken last (null: none since the rewind)
};
