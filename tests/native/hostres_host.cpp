// Host build of csrc/hostres.h and csrc/granule.h for tests/test_hostres_cpu.py: a stand-alone program, built with the address
// and undefined-behaviour sanitizers (LeakSanitizer included) and run as a program.  Not linked against the HIP runtime: the
// raw create / destroy functions are defined HERE over malloc / free -- they count the live resources per family, and the
// k-th creation (of any family) from fail_at(k) on fails -- as are the stubs of hipGetErrorString and fail.  What is checked
// is the ownership: the live counts after every operation and 0 at the end.  Nothing touches a GPU.
#include "granule.h"
#include "hostres.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

static long long g_pinned = 0, g_events = 0, g_streams = 0, g_calls = 0, g_fail_at = 0;
static bool g_fail_mapping = false;
static char g_err[512] = "";
static int g_checks = 0;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) {                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static void fail_at(long long k) { g_fail_at = k; g_calls = 0; }   // 0: no creation fails
static bool injected() { return g_fail_at != 0 && ++g_calls == g_fail_at; }
static long long live() { return g_pinned + g_events + g_streams; }

namespace cfmm {

hipError_t pinned_alloc(void** h, void** d, size_t bytes, bool mapped)
{
    *h = *d = nullptr;
    if (injected() || !(*h = std::malloc(bytes))) return hipErrorOutOfMemory;
    ++g_pinned;
    if (mapped && !g_fail_mapping) *d = *h;
    return hipSuccess;
}
void pinned_free(void* h)
{
    std::free(h);
    --g_pinned;
}
hipError_t event_create(hipEvent_t* e, unsigned)
{
    *e = nullptr;
    if (injected() || !(*e = static_cast<hipEvent_t>(std::malloc(1)))) return hipErrorOutOfMemory;
    ++g_events;
    return hipSuccess;
}
void event_destroy(hipEvent_t e)
{
    std::free(e);
    --g_events;
}
hipError_t stream_create(hipStream_t* s)
{
    *s = nullptr;
    if (injected() || !(*s = static_cast<hipStream_t>(std::malloc(1)))) return hipErrorOutOfMemory;
    ++g_streams;
    return hipSuccess;
}
void stream_destroy(hipStream_t s)
{
    std::free(s);
    --g_streams;
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

extern "C" const char* hipGetErrorString(hipError_t) { return "injected failure"; }

using namespace cfmm;

// An owner with one resource: `make` gives it one, `raw` is what it holds (null: nothing), `count` its family's live count
template <class Owner, class Make, class Raw>
static void check_owner(Make make, Raw raw, const long long& count)
{
    {
        Owner a;
        CHECK(!a && raw(a) == nullptr && count == 0);
        CHECK(make(a) && a && count == 1);
        const void* p = raw(a);
        Owner b(std::move(a));                       // move construction hands the resource over
        CHECK(count == 1 && !a && raw(a) == nullptr && raw(b) == p);
        Owner c;
        CHECK(make(c) && count == 2);
        c = std::move(b);                            // move assignment releases what the target held
        CHECK(count == 1 && !b && raw(c) == p);
        Owner& self = c;
        c = std::move(self);                         // onto itself: nothing happens
        CHECK(count == 1 && raw(c) == p);
        c = std::move(b);                            // from an empty source: the target is released and empty
        CHECK(count == 0 && !c && raw(c) == nullptr);
        CHECK(make(c) && count == 1);
        c.reset();
        CHECK(count == 0 && !c);
        c.reset();                                   // twice: nothing to release
        CHECK(count == 0);
        fail_at(1);
        CHECK(!make(c) && !c && count == 0);        // a failed creation: empty
        fail_at(0);
        CHECK(make(c) && count == 1);
    }                                                // ... and the destructor releases
    CHECK(count == 0 && live() == 0);
}

static void check_pinned()
{
    using Buf = PinnedBuf<double>;
    check_owner<Buf>([](Buf& b) { return b.alloc(nullptr, 5, true) == CFMM_OK && b.dev() == b.host() && b.size() == 5; },
                     [](const Buf& b) { return (const void*)b.host(); }, g_pinned);
    Buf b;
    CHECK(b.alloc(nullptr, 0, true) == CFMM_OK && !b && b.size() == 0 && g_pinned == 0);   // a count of 0: empty
    CHECK(b.alloc(nullptr, 7, false) == CFMM_OK && b.host() && b.dev() == nullptr && g_pinned == 1);   // plain: no device address
    b.host()[6] = 1.0;
    CHECK(b.grow(nullptr, 0, true) == CFMM_OK && b.grow(nullptr, 7, true) == CFMM_OK && b.size() == 7 && b.host()[6] == 1.0);   // has that much: untouched
    CHECK(b.grow(nullptr, 64, true) == CFMM_OK && b.size() == 64 && b.dev() == b.host() && g_pinned == 1);
    b.host()[63] = 2.0;
    // grow frees before it allocates: with the one allocation of a growth failing, nothing is live
    fail_at(1);
    CHECK(b.grow(nullptr, 128, true) == CFMM_ERR_HIP && !b && b.dev() == nullptr && b.size() == 0 && g_pinned == 0);
    CHECK(std::strstr(g_err, "injected failure") != nullptr);
    fail_at(0);
    // a failed mapping leaves a usable host pointer and a null device pointer
    g_fail_mapping = true;
    CHECK(b.alloc(nullptr, 16, true) == CFMM_OK && b && b.dev() == nullptr && b.size() == 16 && g_pinned == 1);
    b.host()[15] = 3.0;
    CHECK(b.host()[15] == 3.0);
    g_fail_mapping = false;
    b.reset();
    CHECK(live() == 0);
}

// With the k-th of its 4 stream + 8 slot + 8 event creations failing: the failed set-up leaves nothing live, a second
// attempt succeeds, and everything is at 0 after destruction
static void check_trade_staging()
{
    constexpr int kT = TradeStaging::kThreads, kS = TradeStaging::kSlots, kAll = kT + 2 * kT * kS;
    static_assert(kAll == 20, "4 streams + 8 slots + 8 events");
    for (int k = 1; k <= kAll; ++k) {
        {
            TradeStaging t;
            fail_at(k);
            CHECK(t.ensure(nullptr) == CFMM_ERR_HIP && !t.ready);
            CHECK(g_calls == k && live() == 0);
            for (int i = 0; i < kT; ++i) {
                CHECK(!t.stream[i]);
                for (int s = 0; s < kS; ++s) CHECK(!t.slot[i][s] && !t.done[i][s]);
            }
            fail_at(0);
            CHECK(t.ensure(nullptr) == CFMM_OK && t.ready);
            CHECK(g_streams == kT && g_pinned == kT * kS && g_events == kT * kS);
            for (int i = 0; i < kT; ++i)
                for (int s = 0; s < kS; ++s) {
                    CHECK(t.slot[i][s].size() == (size_t)TradeStaging::kChunkRows && t.slot[i][s].dev() == nullptr);
                    t.slot[i][s].host()[TradeStaging::kChunkRows - 1] = make_double2(1.0, 2.0);   // (the whole slot is there)
                }
            CHECK(t.ensure(nullptr) == CFMM_OK && live() == kAll);   // ready: creates nothing more
        }
        CHECK(g_streams == 0 && g_pinned == 0 && g_events == 0);
    }
    fail_at(kAll + 1);   // (one past the last creation: the set-up does not notice)
    {
        TradeStaging t;
        CHECK(t.ensure(nullptr) == CFMM_OK && g_calls == kAll);
    }
    fail_at(0);
    CHECK(live() == 0);
}

static unsigned long long bits_of(double x)
{
    unsigned long long u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

static void check_granule()
{
    // the tag of a sequence number: never 0, and the expression every call site used to write out
    const unsigned long long seqs[] = {0ull, 1ull, 0xfffffffeull, 0xffffffffull, 1ull << 32};
    const unsigned long long tags[] = {1ull, 2ull, 0xffffffffull, 1ull, 2ull};
    for (int k = 0; k < 5; ++k) {
        const unsigned long long t = granule_tag(seqs[k]);
        CHECK(t == seqs[k] % 0xffffffffull + 1ull && t == tags[k] && t != 0 && t <= 0xffffffffull);
    }
    // split then reassemble is the identity on the bits
    double nan_payload, denormal;
    const unsigned long long nan_bits = 0x7ff8dead0000beefull, den_bits = 0x0000000000000123ull;
    std::memcpy(&nan_payload, &nan_bits, 8);
    std::memcpy(&denormal, &den_bits, 8);
    const double values[] = {0.0, -0.0, denormal, nan_payload, INFINITY, -INFINITY, 1e-29};
    for (unsigned long long tag : {1ull, 0xffffffffull, 0x12345678ull})
        for (double x : values) {
            const unsigned long long a = granule(tag, x, 0), b = granule(tag, x, 1), u = bits_of(x);
            CHECK(a == (tag << 32 | (u & 0xffffffffull)) && b == (tag << 32 | u >> 32));   // {tag << 32 | 32 bits}, low half first
            CHECK(a == granule_of_bits(tag, u, 0) && b == granule_of_bits(tag, u, 1));
            double y = 42.0;
            CHECK(granule_join(a, b, tag, y) && bits_of(y) == u);
            // a pair with one stale tag is rejected (and leaves the target alone)
            const unsigned long long stale = tag == 1 ? 2 : tag - 1;
            double z = 42.0;
            CHECK(!granule_join(granule(stale, x, 0), b, tag, z) && z == 42.0);
            CHECK(!granule_join(a, granule(stale, x, 1), tag, z) && z == 42.0);
            CHECK(!granule_join(0, 0, tag, z) && z == 42.0);   // an empty buffer carries no tag
        }
}

int main()
{
    check_pinned();
    check_owner<Event>([](Event& e) { return e.create(hipEventDisableTiming) == hipSuccess && e.create() == hipSuccess; },   // (an existing one is kept)
                       [](const Event& e) { return (const void*)e.get(); }, g_events);
    check_owner<Stream>([](Stream& s) { return s.create() == hipSuccess && s.create() == hipSuccess; },
                        [](const Stream& s) { return (const void*)s.get(); }, g_streams);
    check_trade_staging();
    check_granule();
    CHECK(live() == 0);
    std::printf("HOSTRES_OK %d checks\n", g_checks);
    return 0;
}
