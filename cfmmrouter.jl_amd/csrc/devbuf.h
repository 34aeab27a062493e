// devbuf.h -- internal: DevBuf<T>, the one owner of a device array.  Host-side only.
// The rule it carries: a DevBuf ALWAYS owns what it points to -- it frees in its destructor, a move hands the array over,
// nothing copies it -- and a device view struct (sweep.h: ProductPools, UniV3Pools, NCoinPools, ScatterArgs, ...) NEVER
// does: a view takes `.get()` for the length of one launch.  Every allocation and release goes through dev_alloc /
// dev_alloc_fine / dev_free (abi_context.cpp), the only callers of hipMalloc / hipExtMallocWithFlags / hipFree for the
// library's own arrays.  (The owners of pinned memory, events and streams: hostres.h.)
#pragma once

#include "../../include/cfmm_amd.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cfmm {

int fail(const cfmm_ctx* c, int code, const char* fmt, ...);

// abi_context.cpp
hipError_t dev_alloc(void** p, size_t bytes);   // *p = nullptr on failure
hipError_t dev_alloc_fine(void** p, size_t bytes);   // the same in FINE-GRAINED device memory (the host writes it through the PCIe BAR)
void dev_free(void* p);
// counts every create and release of a device array or pinned buffer of the library (process-wide, monotonic): whoever
// caches device addresses -- the sweep descriptors, abi_sweep.cpp ensure_desc -- compares it to know that none has gone
uint64_t resource_epoch();

template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;   // elements

public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

    void reset()
    {
        if (p_) dev_free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    // `count` elements, contents undefined; what it held goes FIRST (never both at once).  count == 0, or a failure
    // (CFMM_ERR_HIP): empty.
    int alloc(const cfmm_ctx* c, size_t count)
    {
        reset();
        if (count == 0) return CFMM_OK;
        void* p = nullptr;
        const hipError_t e = dev_alloc(&p, count * sizeof(T));
        if (e != hipSuccess) return fail(c, CFMM_ERR_HIP, "device allocation of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        p_ = static_cast<T*>(p);
        n_ = count;
        return CFMM_OK;
    }
    // `count` elements of fine-grained memory.  Optional wherever it is used: a failure leaves the buffer empty and sets no error
    bool alloc_fine(size_t count)
    {
        reset();
        void* p = nullptr;
        if (count == 0 || dev_alloc_fine(&p, count * sizeof(T)) != hipSuccess) return false;
        p_ = static_cast<T*>(p);
        n_ = count;
        return true;
    }
    // alloc + a blocking copy of `count` elements from the host
    int upload(const cfmm_ctx* c, const void* src, size_t count)
    {
        const int rc = alloc(c, count);
        if (rc != CFMM_OK || count == 0) return rc;
        const hipError_t e = hipMemcpy(p_, src, count * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) return CFMM_OK;
        reset();
        return fail(c, CFMM_ERR_HIP, "upload of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    // room for at least `count` elements: untouched when it has that much, else alloc (the old contents are DISCARDED --
    // every growable buffer of the library is rewritten by its next user)
    int grow(const cfmm_ctx* c, size_t count) { return count <= n_ ? CFMM_OK : alloc(c, count); }
};

} // namespace cfmm
