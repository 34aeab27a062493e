// find_out_checks_host.cpp -- TEST-ONLY host build of csrc/find_checks.h as cfmm_find_path_out calls it: check_find with the
// entry's own name and "amount_out" as the name of the given amount.  Two uses (tests/test_find_path_out_cpu.py), as
// find_checks_host.cpp: built as a shared object and loaded with ctypes (find_out_checks_host: one call on the caller's arrays;
// find_out_checks_host_cases: the case list below), and built with -DFIND_OUT_CHECKS_HOST_MAIN under the address and
// undefined-behaviour sanitizers as a stand-alone program that runs the same case list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/find_checks.h"

namespace {
constexpr const char* kWho = "cfmm_find_path_out";
constexpr const char* kAmount = "amount_out";
}

// outputs != 0: every output array is given (the check only looks at whether they are null)
extern "C" int find_out_checks_host(int64_t n_tokens, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                                    const double* amount_out, int outputs, char* msg, int64_t len)
{
    static int some;
    const void* o = outputs ? &some : nullptr;
    return cfmm::check_find(kWho, n_tokens, count, max_hops, token_in, token_out, amount_out, o, o, o, o, o, o, o, msg, (size_t)len, kAmount);
}

namespace {

// a valid batch of 6 queries on a market of 10 tokens; query 0 wants exactly 0 and query 5 pays in the token it buys
struct Batch {
    static constexpr int64_t count = 6;
    std::vector<int32_t> tin{0, 1, 2, 9, 4, 5}, tout{9, 0, 3, 1, 2, 5};
    std::vector<double> amt{0.0, 0.5, 1.0, 1.5, 2.0, 2.5};
    int dummy = 0;
    int check(char* msg, size_t len, int32_t max_hops = 3, int64_t n = count, int null_at = -1) const
    {
        const void* p[10] = {tin.data(), tout.data(), amt.data(), &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy};
        if (null_at >= 0) p[null_at] = nullptr;
        return cfmm::check_find(kWho, 10, n, max_hops, static_cast<const int32_t*>(p[0]), static_cast<const int32_t*>(p[1]),
                                static_cast<const double*>(p[2]), p[3], p[4], p[5], p[6], p[7], p[8], p[9], msg, len, kAmount);
    }
};

int expect(const char* what, int rc, const char* msg, int want_rc, const char* want_text)
{
    const bool ok = rc == want_rc && (want_text == nullptr || std::strstr(msg, want_text) != nullptr);
    if (!ok) std::printf("FAILED %s: rc %d, message '%s' (wanted rc %d, '%s')\n", what, rc, msg, want_rc, want_text ? want_text : "");
    return ok ? 0 : 1;
}

} // namespace

// the case list; returns the number of cases that did not behave
extern "C" int find_out_checks_host_cases()
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
        bad += expect("count 0 with null arrays", cfmm::check_find(kWho, 10, 0, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                   nullptr, nullptr, nullptr, msg, sizeof msg, kAmount), msg, CFMM_OK, nullptr);
    }
    { Batch b; bad += expect("count < 0", b.check(msg, sizeof msg, 3, -1), msg, E, "cfmm_find_path_out: count must be >= 0"); }
    { Batch b; bad += expect("max_hops 0", b.check(msg, sizeof msg, 0), msg, E, "cfmm_find_path_out: max_hops must be 1 .. 8 (got 0)"); }
    { Batch b; bad += expect("max_hops 9", b.check(msg, sizeof msg, 9), msg, E, "cfmm_find_path_out: max_hops must be 1 .. 8 (got 9)"); }
    { Batch b; bad += expect("max_hops is judged before the arrays", b.check(msg, sizeof msg, 9, Batch::count, 0), msg, E, "max_hops"); }
    for (int k = 0; k < 10; ++k) {
        Batch b;
        bad += expect("a null array", b.check(msg, sizeof msg, 3, Batch::count, k), msg, E, "cfmm_find_path_out: null query array");
    }
    { Batch b; b.tin[3] = 10; bad += expect("token_in", b.check(msg, sizeof msg), msg, E, "cfmm_find_path_out: query 3: token_in 10 out of range (the market has 10 tokens)"); }
    { Batch b; b.tin[0] = -1; bad += expect("token_in < 0", b.check(msg, sizeof msg), msg, E, "query 0: token_in -1 out of range"); }
    { Batch b; b.tout[5] = 77; bad += expect("token_out", b.check(msg, sizeof msg), msg, E, "cfmm_find_path_out: query 5: token_out 77 out of range (the market has 10 tokens)"); }
    { Batch b; b.tout[2] = -3; bad += expect("token_out < 0", b.check(msg, sizeof msg), msg, E, "query 2: token_out -3"); }
    { Batch b; b.amt[4] = -1.0; bad += expect("negative amount", b.check(msg, sizeof msg), msg, E, "cfmm_find_path_out: query 4: amount_out must be finite and >= 0"); }
    { Batch b; b.amt[1] = std::numeric_limits<double>::quiet_NaN(); bad += expect("NaN amount", b.check(msg, sizeof msg), msg, E, "query 1: amount_out"); }
    { Batch b; b.amt[5] = std::numeric_limits<double>::infinity(); bad += expect("inf amount", b.check(msg, sizeof msg), msg, E, "query 5: amount_out"); }
    { Batch b; b.amt[0] = -0.0; bad += expect("-0.0 is an amount", b.check(msg, sizeof msg), msg, CFMM_OK, nullptr); }
    { Batch b; b.amt[5] = -1.0; b.tout[2] = 10; bad += expect("the first bad query is named", b.check(msg, sizeof msg), msg, E, "query 2: token_out"); }
    { Batch b; b.tin[4] = 10; bad += expect("a query beyond count is not looked at", b.check(msg, sizeof msg, 3, 4), msg, CFMM_OK, nullptr); }
    // no refusal of this entry speaks of amount_in, and the exact-input entry's text is what it was
    { Batch b; b.amt[2] = -1.0; b.check(msg, sizeof msg); bad += expect("the other amount is not named", std::strstr(msg, "amount_in") != nullptr, msg, 0, nullptr); }
    {
        Batch b;
        b.amt[2] = -1.0;
        const int rc = cfmm::check_find("cfmm_find_path", 10, Batch::count, 3, b.tin.data(), b.tout.data(), b.amt.data(), &b.dummy, &b.dummy, &b.dummy,
                                        &b.dummy, &b.dummy, &b.dummy, &b.dummy, msg, sizeof msg);
        bad += expect("the defaulted name", rc, msg, E, "cfmm_find_path: query 2: amount_in must be finite and >= 0");
    }
    return bad;
}

#ifdef FIND_OUT_CHECKS_HOST_MAIN
int main()
{
    const int bad = find_out_checks_host_cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("FIND_OUT_CHECKS_HOST_OK\n");
    return 0;
}
#endif
