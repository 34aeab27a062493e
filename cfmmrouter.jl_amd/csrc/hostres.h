// hostres.h -- internal: the owners of what is not a device array -- PinnedBuf<T> (pinned host memory, mapped or plain),
// Event, Stream -- and EventPairs and TradeStaging, which are built from them.  Host-side only.
// The rule is devbuf.h's: an owner ALWAYS owns what it holds -- it releases in its destructor, a move hands the resource
// over, nothing copies it -- and whoever takes `.host()` / `.dev()` / `.get()` never does.  Every create and destroy goes
// through the functions below (abi_context.cpp, beside dev_alloc / dev_free), the only callers of hipHostMalloc /
// hipHostFree / hipHostGetDevicePointer, hipEventCreateWithFlags / hipEventDestroy and hipStreamCreateWithFlags /
// hipStreamDestroy for the library's own resources.
#pragma once

#include "devbuf.h"

#include <vector>

namespace cfmm {

// abi_context.cpp
hipError_t pinned_alloc(void** h, void** d, size_t bytes, bool mapped);   // *h = nullptr on failure; *d = nullptr when not
                                                                          // mapped, or when the mapping failed (h stays usable)
void pinned_free(void* h);
hipError_t event_create(hipEvent_t* e, unsigned flags);                   // *e = nullptr on failure
void event_destroy(hipEvent_t e);
hipError_t stream_create(hipStream_t* s);                                 // non-blocking; *s = nullptr on failure
void stream_destroy(hipStream_t s);

template <class T>
class PinnedBuf {
    T* h_ = nullptr;
    T* d_ = nullptr;   // device address of h_, or null
    size_t n_ = 0;     // elements

public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : h_(o.h_), d_(o.d_), n_(o.n_) { o.h_ = o.d_ = nullptr; o.n_ = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = o.h_; d_ = o.d_; n_ = o.n_;
            o.h_ = o.d_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }

    T* host() const { return h_; }
    T* dev() const { return d_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return h_ != nullptr; }

    void reset()
    {
        if (h_) pinned_free(h_);
        h_ = d_ = nullptr;
        n_ = 0;
    }
    // `count` elements, contents undefined; what it held goes FIRST.  count == 0, or a failure (CFMM_ERR_HIP): empty.
    // mapped: dev() is the device's address of the same memory -- or null when the mapping failed, which is NOT a failure
    // here (host() is usable; the caller decides whether it can do without)
    int alloc(const cfmm_ctx* c, size_t count, bool mapped)
    {
        reset();
        if (count == 0) return CFMM_OK;
        void *h = nullptr, *d = nullptr;
        const hipError_t e = pinned_alloc(&h, &d, count * sizeof(T), mapped);
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "hipHostMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        h_ = static_cast<T*>(h);
        d_ = static_cast<T*>(d);
        n_ = count;
        return CFMM_OK;
    }
    // room for at least `count` elements: untouched when it has that much, else alloc (the old contents are DISCARDED)
    int grow(const cfmm_ctx* c, size_t count, bool mapped) { return count <= n_ ? CFMM_OK : alloc(c, count, mapped); }
};

// A HIP event / stream, created on request and destroyed with the object
class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept
    {
        if (this != &o) {
            reset();
            e_ = o.e_;
            o.e_ = nullptr;
        }
        return *this;
    }
    ~Event() { reset(); }

    hipEvent_t get() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
    void reset()
    {
        if (e_) event_destroy(e_);
        e_ = nullptr;
    }
    // the event exists afterwards (one that exists already is kept); flags: hipEventDefault (timing) / hipEventDisableTiming
    hipError_t create(unsigned flags = hipEventDefault) { return e_ ? hipSuccess : event_create(&e_, flags); }
    int create(const cfmm_ctx* c, unsigned flags)   // the same, with the error text set
    {
        const hipError_t e = create(flags);
        return e == hipSuccess ? CFMM_OK : fail(c, CFMM_ERR_HIP, "hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
    }
};

// The {start, stop} pairs that time the query entries' launches under option "time_kernels", created on demand and kept
struct EventPairs {
    std::vector<Event> ev;   // pair j: ev[2j], ev[2j + 1]
    // pairs first .. k - 1 exist afterwards
    int ensure(const cfmm_ctx* c, size_t k, size_t first = 0)
    {
        if (ev.size() < 2 * k) ev.resize(2 * k);
        for (size_t i = 2 * first; i < 2 * k; ++i)
            if (const int rc = ev[i].create(c, hipEventDefault)) return rc;
        return CFMM_OK;
    }
    // what a launch takes: pair j, or nulls (an untimed launch) when timing is off
    hipEvent_t start(size_t j, bool on = true) const { return on ? ev[2 * j].get() : nullptr; }
    hipEvent_t stop(size_t j, bool on = true) const { return on ? ev[2 * j + 1].get() : nullptr; }
    // the spans of pairs first .. first + k - 1, whose events have all been reached, summed, in nanoseconds
    int elapsed_ns(const cfmm_ctx* c, size_t first, size_t k, int64_t& ns) const
    {
        double ms_sum = 0.0;
        for (size_t j = first; j < first + k; ++j) {
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, start(j), stop(j));
            if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "reading a kernel's span from its events failed: %s", hipGetErrorString(e));
            ms_sum += (double)ms;
        }
        ns = (int64_t)(ms_sum * 1e6);
        return CFMM_OK;
    }
};

class Stream {
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    Stream& operator=(Stream&& o) noexcept
    {
        if (this != &o) {
            reset();
            s_ = o.s_;
            o.s_ = nullptr;
        }
        return *this;
    }
    ~Stream() { reset(); }

    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    void reset()
    {
        if (s_) stream_destroy(s_);
        s_ = nullptr;
    }
    hipError_t create() { return s_ ? hipSuccess : stream_create(&s_); }   // (hipStreamNonBlocking)
    int create(const cfmm_ctx* c)
    {
        const hipError_t e = create();
        return e == hipSuccess ? CFMM_OK : fail(c, CFMM_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
    }
};

// Pinned staging of the trade download (abi_trades.cpp): a few worker threads, each with its own stream and two slots.
struct TradeStaging {
    static constexpr int kThreads = 4, kSlots = 2;
    static constexpr int64_t kChunkRows = 1 << 16;   // 1 MiB per slot
    PinnedBuf<double2> slot[kThreads][kSlots];
    Stream stream[kThreads];
    Event done[kThreads][kSlots];
    bool ready = false;

    // everything or nothing: a set-up that fails part-way releases what it had created, and the next call starts afresh
    int ensure(const cfmm_ctx* c)
    {
        if (ready) return CFMM_OK;
        const int rc = create(c);
        if (rc != CFMM_OK) *this = TradeStaging();
        ready = rc == CFMM_OK;
        return rc;
    }

private:
    int create(const cfmm_ctx* c)
    {
        int rc;
        for (int k = 0; k < kThreads; ++k) {
            if ((rc = stream[k].create(c)) != CFMM_OK) return rc;
            for (int s = 0; s < kSlots; ++s)
                if ((rc = slot[k][s].alloc(c, (size_t)kChunkRows, false)) || (rc = done[k][s].create(c, hipEventDisableTiming))) return rc;
        }
        return CFMM_OK;
    }
};

} // namespace cfmm
