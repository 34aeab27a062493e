// find_checks_host.cpp -- TEST-ONLY host build of csrc/find_checks.h, the HIP-free checks cfmm_find_path applies to a batch of
// queries before anything is enqueued, and its chunking rule.  Two uses (tests/test_find_path_cpu.py): built as a shared object
// and loaded with ctypes (find_checks_host: one call of check_find on the caller's arrays; find_checks_host_chunk: the chunking
// rule; find_checks_host_cases: the case list below), and built with -DFIND_CHECKS_HOST_MAIN under the address and
// undefined-behaviour sanitizers as a stand-alone program that runs the same case list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/find_checks.h"

// outputs != 0: every output array is given (the check only looks at whether they are null)
extern "C" int find_checks_host(int64_t n_tokens, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                                const double* amount_in, int outputs, char* msg, int64_t len)
{
    static int some;
    const void* o = outputs ? &some : nullptr;
    return cfmm::check_find("cfmm_find_path", n_tokens, count, max_hops, token_in, token_out, amount_in, o, o, o, o, o, o, o, msg, (size_t)len);
}

extern "C" int64_t find_checks_host_chunk(int64_t n_tokens, int32_t max_hops) { return cfmm::find_chunk_queries(n_tokens, max_hops); }

namespace {

// a valid batch of 6 queries on a market of 10 tokens; query 0 tenders exactly 0 and query 5 asks for its own token back
struct Batch {
    static constexpr int64_t count = 6;
    std::vector<int32_t> tin{0, 1, 2, 9, 4, 5}, tout{9, 0, 3, 1, 2, 5};
    std::vector<double> amt{0.0, 0.5, 1.0, 1.5, 2.0, 2.5};
    int dummy = 0;
    int check(char* msg, size_t len, int32_t max_hops = 3, int64_t n = count, int null_at = -1) const
    {
        const void* p[10] = {tin.data(), tout.data(), amt.data(), &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy};
        if (null_at >= 0) p[null_at] = nullptr;
        return cfmm::check_find("cfmm_find_path", 10, n, max_hops, static_cast<const int32_t*>(p[0]), static_cast<const int32_t*>(p[1]),
                                static_cast<const double*>(p[2]), p[3], p[4], p[5], p[6], p[7], p[8], p[9], msg, len);
    }
};

int expect(const char* what, int rc, const char* msg, int want_rc, const char* want_text)
{
    const bool ok = rc == want_rc && (want_text == nullptr || std::strstr(msg, want_text) != nullptr);
    if (!ok) std::printf("FAILED %s: rc %d, message '%s' (wanted rc %d, '%s')\n", what, rc, msg, want_rc, want_text ? want_text : "");
    return ok ? 0 : 1;
}

int expect_eq(const char* what, int64_t got, int64_t want)
{
    if (got != want) std::printf("FAILED %s: %lld (wanted %lld)\n", what, (long long)got, (long long)want);
    return got == want ? 0 : 1;
}

} // namespace

// the case list; returns the number of cases that did not behave
extern "C" int find_checks_host_cases()
{
    int bad = 0;
    char msg[256];
    const int E = CFMM_ERR_INVALID_ARG;
    {
        Batch b;
        msg[0] = 0;
        bad += expect("valid batch", b.check(msg, sizeof msg), msg, CFMM_OK, nullptr);
        bad += expect("valid batch leaves the message alone", msg[0], msg, 0, nullptr);
        bad += expect("max_hops 1", b.check(msg, sizeof msg, 1), msg, CFMM_OK, nullptr);
        bad += expect("max_hops 8", b.check(msg, sizeof msg, 8), msg, CFMM_OK, nullptr);
        bad += expect("count 0 with null arrays", cfmm::check_find("cfmm_find_path", 10, 0, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                   nullptr, nullptr, nullptr, nullptr, msg, sizeof msg), msg, CFMM_OK, nullptr);
    }
    { Batch b; bad += expect("count < 0", b.check(msg, sizeof msg, 3, -1), msg, E, "cfmm_find_path: count must be >= 0"); }
    { Batch b; bad += expect("max_hops 0", b.check(msg, sizeof msg, 0), msg, E, "cfmm_find_path: max_hops must be 1 .. 8 (got 0)"); }
    { Batch b; bad += expect("max_hops 9", b.check(msg, sizeof msg, 9), msg, E, "cfmm_find_path: max_hops must be 1 .. 8 (got 9)"); }
    { Batch b; bad += expect("max_hops is judged before the arrays", b.check(msg, sizeof msg, 9, Batch::count, 0), msg, E, "max_hops"); }
    for (int k = 0; k < 10; ++k) {
        Batch b;
        bad += expect("a null array", b.check(msg, sizeof msg, 3, Batch::count, k), msg, E, "cfmm_find_path: null query array");
    }
    { Batch b; b.tin[3] = 10; bad += expect("token_in", b.check(msg, sizeof msg), msg, E, "cfmm_find_path: query 3: token_in 10 out of range (the market has 10 tokens)"); }
    { Batch b; b.tin[0] = -1; bad += expect("token_in < 0", b.check(msg, sizeof msg), msg, E, "query 0: token_in -1 out of range"); }
    { Batch b; b.tout[5] = 77; bad += expect("token_out", b.check(msg, sizeof msg), msg, E, "cfmm_find_path: query 5: token_out 77 out of range (the market has 10 tokens)"); }
    { Batch b; b.tout[2] = -3; bad += expect("token_out < 0", b.check(msg, sizeof msg), msg, E, "query 2: token_out -3"); }
    { Batch b; b.amt[4] = -1.0; bad += expect("negative amount", b.check(msg, sizeof msg), msg, E, "cfmm_find_path: query 4: amount_in must be finite and >= 0"); }
    { Batch b; b.amt[1] = std::numeric_limits<double>::quiet_NaN(); bad += expect("NaN amount", b.check(msg, sizeof msg), msg, E, "query 1: amount_in"); }
    { Batch b; b.amt[5] = std::numeric_limits<double>::infinity(); bad += expect("inf amount", b.check(msg, sizeof msg), msg, E, "query 5: amount_in"); }
    { Batch b; b.amt[0] = -0.0; bad += expect("-0.0 is an amount", b.check(msg, sizeof msg), msg, CFMM_OK, nullptr); }
    { Batch b; b.amt[5] = -1.0; b.tout[2] = 10; bad += expect("the first bad query is named", b.check(msg, sizeof msg), msg, E, "query 2: token_out"); }
    { Batch b; b.tin[4] = 10; bad += expect("a query beyond count is not looked at", b.check(msg, sizeof msg, 3, 4), msg, CFMM_OK, nullptr); }
    // the chunking rule: (max_hops + 1) x queries x n_tokens x 8 bytes within 256 MiB, at least one query
    bad += expect_eq("the budget", cfmm::kFindScratchBudget, 256ll << 20);
    bad += expect_eq("65536 tokens, 3 hops", cfmm::find_chunk_queries(65536, 3), 128);
    bad += expect_eq("65536 tokens, 8 hops", cfmm::find_chunk_queries(65536, 8), 56);
    bad += expect_eq("a market over the budget still runs", cfmm::find_chunk_queries(100000000, 8), 1);
    bad += expect_eq("few tokens: the grid's limit", cfmm::find_chunk_queries(2, 1), cfmm::kFindMaxChunk);
    bad += expect_eq("64 tokens, 8 hops", cfmm::find_chunk_queries(64, 8), (256ll << 20) / (9 * 64 * 8));
    return bad;
}

#ifdef FIND_CHECKS_HOST_MAIN
int main()
{
    const int bad = find_checks_host_cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("FIND_CHECKS_HOST_OK\n");
    return 0;
}
#endif
