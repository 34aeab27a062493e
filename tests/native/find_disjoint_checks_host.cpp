// find_disjoint_checks_host.cpp -- TEST-ONLY stand-alone host program over csrc/find_checks.h: the HIP-free checks
// cfmm_find_disjoint_paths applies before anything is enqueued (check_find_disjoint) and its chunking rule
// (find_disjoint_chunk_queries).  tests/test_find_disjoint_cpu.py builds it twice -- plainly, and with
// -fsanitize=address,undefined -- and runs it as a program:
//   (no argument)   the case list below: every refusal text; prints FIND_DISJOINT_CHECKS_HOST_OK
//   chunks          one line "n_tokens max_hops pools budget chunk" per point of a grid, for the test to judge the rule
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/find_checks.h"

namespace {

const char* const kWho = "cfmm_find_disjoint_paths";

// a valid batch of 6 queries on a market of 10 tokens; query 0 tenders exactly 0 and query 5 asks for its own token back
struct Batch {
    static constexpr int64_t count = 6;
    std::vector<int32_t> tin{0, 1, 2, 9, 4, 5}, tout{9, 0, 3, 1, 2, 5};
    std::vector<double> amt{0.0, 0.5, 1.0, 1.5, 2.0, 2.5};
    int dummy = 0;
    // null_at: 0 .. 2 the inputs, 3 n_paths, 4 .. 10 amount_out, n_hops, status and the four hop arrays
    int check(char* msg, size_t len, int32_t max_paths = 4, int32_t max_hops = 3, int64_t n = count, int null_at = -1) const
    {
        const void* p[11] = {tin.data(), tout.data(), amt.data(), &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy};
        if (null_at >= 0) p[null_at] = nullptr;
        return cfmm::check_find_disjoint(kWho, 10, n, max_paths, max_hops, static_cast<const int32_t*>(p[0]), static_cast<const int32_t*>(p[1]),
                                         static_cast<const double*>(p[2]), p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], msg, len);
    }
};

int expect(const char* what, int rc, const char* msg, int want_rc, const char* want_text)
{
    const bool ok = rc == want_rc && (want_text == nullptr || std::strcmp(msg, want_text) == 0);
    if (!ok) std::printf("FAILED %s: rc %d, message '%s' (wanted rc %d, '%s')\n", what, rc, msg, want_rc, want_text ? want_text : "");
    return ok ? 0 : 1;
}

int expect_eq(const char* what, int64_t got, int64_t want)
{
    if (got != want) std::printf("FAILED %s: %lld (wanted %lld)\n", what, (long long)got, (long long)want);
    return got == want ? 0 : 1;
}

int cases()
{
    int bad = 0;
    char msg[256];
    const int E = CFMM_ERR_INVALID_ARG;
    {
        Batch b;
        msg[0] = 0;
        bad += expect("valid batch", b.check(msg, sizeof msg), msg, CFMM_OK, "");
        for (int32_t k = 1; k <= CFMM_MAX_SPLIT_PATHS; ++k) bad += expect("max_paths 1 .. 8", b.check(msg, sizeof msg, k), msg, CFMM_OK, "");
        bad += expect("max_hops 1", b.check(msg, sizeof msg, 4, 1), msg, CFMM_OK, "");
        bad += expect("max_hops 8", b.check(msg, sizeof msg, 4, 8), msg, CFMM_OK, "");
        bad += expect("count 0 with null arrays", cfmm::check_find_disjoint(kWho, 10, 0, 4, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                                            nullptr, nullptr, nullptr, nullptr, nullptr, msg, sizeof msg), msg, CFMM_OK, "");
    }
    { Batch b; bad += expect("count < 0", b.check(msg, sizeof msg, 4, 3, -1), msg, E, "cfmm_find_disjoint_paths: count must be >= 0"); }
    { Batch b; bad += expect("max_paths 0", b.check(msg, sizeof msg, 0), msg, E, "cfmm_find_disjoint_paths: max_paths must be 1 .. 8 (got 0)"); }
    { Batch b; bad += expect("max_paths 9", b.check(msg, sizeof msg, 9), msg, E, "cfmm_find_disjoint_paths: max_paths must be 1 .. 8 (got 9)"); }
    { Batch b; bad += expect("max_paths -1", b.check(msg, sizeof msg, -1), msg, E, "cfmm_find_disjoint_paths: max_paths must be 1 .. 8 (got -1)"); }
    { Batch b; bad += expect("max_paths of an empty call", b.check(msg, sizeof msg, 9, 3, 0), msg, E, "cfmm_find_disjoint_paths: max_paths must be 1 .. 8 (got 9)"); }
    { Batch b; bad += expect("max_hops 0", b.check(msg, sizeof msg, 4, 0), msg, E, "cfmm_find_disjoint_paths: max_hops must be 1 .. 8 (got 0)"); }
    { Batch b; bad += expect("max_hops 9", b.check(msg, sizeof msg, 4, 9), msg, E, "cfmm_find_disjoint_paths: max_hops must be 1 .. 8 (got 9)"); }
    { Batch b; bad += expect("the scalars are judged before the arrays", b.check(msg, sizeof msg, 0, 3, Batch::count, 0), msg, E, "cfmm_find_disjoint_paths: max_paths must be 1 .. 8 (got 0)"); }
    for (int k = 0; k < 11; ++k) {   // n_paths (3) among them
        Batch b;
        bad += expect("a null array", b.check(msg, sizeof msg, 4, 3, Batch::count, k), msg, E, "cfmm_find_disjoint_paths: null query array");
    }
    { Batch b; b.tin[3] = 10; bad += expect("token_in", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 3: token_in 10 out of range (the market has 10 tokens)"); }
    { Batch b; b.tin[0] = -1; bad += expect("token_in < 0", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 0: token_in -1 out of range (the market has 10 tokens)"); }
    { Batch b; b.tout[5] = 77; bad += expect("token_out", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 5: token_out 77 out of range (the market has 10 tokens)"); }
    { Batch b; b.tout[2] = -3; bad += expect("token_out < 0", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 2: token_out -3 out of range (the market has 10 tokens)"); }
    { Batch b; b.amt[4] = -1.0; bad += expect("negative amount", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 4: amount_in must be finite and >= 0"); }
    { Batch b; b.amt[1] = std::numeric_limits<double>::quiet_NaN(); bad += expect("NaN amount", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 1: amount_in must be finite and >= 0"); }
    { Batch b; b.amt[5] = std::numeric_limits<double>::infinity(); bad += expect("inf amount", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 5: amount_in must be finite and >= 0"); }
    { Batch b; b.amt[0] = -0.0; msg[0] = 0; bad += expect("-0.0 is an amount", b.check(msg, sizeof msg), msg, CFMM_OK, ""); }
    { Batch b; b.amt[5] = -1.0; b.tout[2] = 10; bad += expect("the first bad query is named", b.check(msg, sizeof msg), msg, E, "cfmm_find_disjoint_paths: query 2: token_out 10 out of range (the market has 10 tokens)"); }
    { Batch b; b.tin[4] = 10; msg[0] = 0; bad += expect("a query beyond count is not looked at", b.check(msg, sizeof msg, 4, 3, 4), msg, CFMM_OK, ""); }
    // the chunking rule: ((max_hops + 1) x n_tokens + ceil(pools / 64)) x 8 bytes per query within 256 MiB, at least one query
    bad += expect_eq("ban words of 2056 pools", cfmm::find_ban_words(2056), 33);
    bad += expect_eq("ban words of 64 pools", cfmm::find_ban_words(64), 1);
    bad += expect_eq("ban words of 65 pools", cfmm::find_ban_words(65), 2);
    bad += expect_eq("ban words of no pool", cfmm::find_ban_words(0), 1);
    bad += expect_eq("few pools: one word beside the layers", cfmm::find_disjoint_chunk_queries(65536, 8, 64), (256ll << 20) / ((9 * 65536 + 1) * 8));
    bad += expect_eq("65536 tokens, 8 hops, 1028 pools", cfmm::find_disjoint_chunk_queries(65536, 8, 1028), 56);
    bad += expect_eq("a million pools on 4096 tokens, 3 hops", cfmm::find_disjoint_chunk_queries(4096, 3, 1000000), (256ll << 20) / ((4 * 4096 + 15625) * 8));
    bad += expect_eq("a market over the budget still runs", cfmm::find_disjoint_chunk_queries(100000000, 8, 1000), 1);
    bad += expect_eq("pools over the budget still run", cfmm::find_disjoint_chunk_queries(2, 1, 1ll << 40), 1);
    bad += expect_eq("few tokens and pools: the grid's limit", cfmm::find_disjoint_chunk_queries(2, 1, 10), cfmm::kFindMaxChunk);
    return bad;
}

void chunks()
{
    const int64_t tokens[] = {1, 2, 65, 4096, 65536, 1000000, 100000000};
    const int64_t pools[] = {0, 1, 64, 65, 2056, 1000000, 1000000000, 1ll << 40};
    const int64_t budgets[] = {1, 4096, 1 << 20, cfmm::kFindScratchBudget};
    for (int64_t t : tokens)
        for (int32_t h = 1; h <= CFMM_MAX_PATH_HOPS; ++h)
            for (int64_t p : pools)
                for (int64_t b : budgets)
                    std::printf("%lld %d %lld %lld %lld\n", (long long)t, (int)h, (long long)p, (long long)b,
                                (long long)cfmm::find_disjoint_chunk_queries(t, h, p, b));
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "chunks")) {
        chunks();
        return 0;
    }
    const int bad = cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("FIND_DISJOINT_CHECKS_HOST_OK\n");
    return 0;
}
