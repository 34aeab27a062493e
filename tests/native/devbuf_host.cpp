// Host build of csrc/devbuf.h for tests/test_devbuf_cpu.py: DevBuf<double> over malloc / free.  Not linked against the HIP
// runtime: dev_alloc / dev_alloc_fine / dev_free are defined HERE (they count the live allocations, and the k-th allocation from
// devbuf_fail_at(k) on fails), as are the stubs of hipMemcpy, hipGetErrorString and fail.  Nothing touches a GPU.
#include "devbuf.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

static long long g_live = 0, g_calls = 0, g_fail_at = 0;
static char g_err[512] = "";

namespace cfmm {

hipError_t dev_alloc(void** p, size_t bytes)
{
    *p = nullptr;
    if (g_fail_at != 0 && ++g_calls == g_fail_at) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    if (!*p) return hipErrorOutOfMemory;
    ++g_live;
    return hipSuccess;
}

hipError_t dev_alloc_fine(void** p, size_t bytes) { return dev_alloc(p, bytes); }   // (the same counter and the same injected failures)

void dev_free(void* p)
{
    std::free(p);
    --g_live;
}

int fail(const cfmm_ctx*, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

} // namespace cfmm

using Buf = cfmm::DevBuf<double>;

extern "C" {

hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind)
{
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "injected failure"; }

long long devbuf_live() { return g_live; }
void devbuf_fail_at(long long k) { g_fail_at = k; g_calls = 0; }   // 0: no allocation fails
const char* devbuf_last_error() { return g_err; }

Buf* devbuf_new() { return new Buf(); }
void devbuf_delete(Buf* b) { delete b; }
Buf* devbuf_move_new(Buf* src) { return new Buf(std::move(*src)); }
void devbuf_move_assign(Buf* dst, Buf* src) { *dst = std::move(*src); }
int devbuf_alloc(Buf* b, long long n) { return b->alloc(nullptr, (size_t)n); }
int devbuf_alloc_fine(Buf* b, long long n) { return b->alloc_fine((size_t)n) ? 1 : 0; }
int devbuf_upload(Buf* b, const double* src, long long n) { return b->upload(nullptr, src, (size_t)n); }
int devbuf_grow(Buf* b, long long n) { return b->grow(nullptr, (size_t)n); }
void devbuf_reset(Buf* b) { b->reset(); }
long long devbuf_size(const Buf* b) { return (long long)b->size(); }
double* devbuf_get(const Buf* b) { return b->get(); }
int devbuf_bool(const Buf* b) { return *b ? 1 : 0; }

// four uploads into four buffers of one scope, chained the way the upload paths chain them (abi_upload.cpp); *live_inside:
// the live count before the scope ends
int devbuf_four_uploads(const double* src, long long n, long long* live_inside)
{
    Buf a, b, c, d;
    int rc;
    if ((rc = a.upload(nullptr, src, (size_t)n)) || (rc = b.upload(nullptr, src, (size_t)n)) ||
        (rc = c.upload(nullptr, src, (size_t)n)) || (rc = d.upload(nullptr, src, (size_t)n))) {
        *live_inside = g_live;
        return rc;
    }
    *live_inside = g_live;
    return CFMM_OK;
}

} // extern "C"
