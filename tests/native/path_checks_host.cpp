// path_checks_host.cpp -- TEST-ONLY host build of csrc/path_checks.h, the HIP-free checks cfmm_quote_path / cfmm_quote_path_out
// apply to a batch of paths before anything is enqueued.  Two uses (tests/test_quote_path_cpu.py): built as a shared object
// and loaded with ctypes (path_checks_host: one call of check_paths on the caller's arrays; path_checks_host_cases: the case
// list below), and built with -DPATH_CHECKS_HOST_MAIN under the address and undefined-behaviour sanitizers as a stand-alone
// program that runs the same case list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/path_checks.h"

extern "C" int path_checks_host(int64_t nseg, const int32_t* kind, const int64_t* m, const int32_t* n_coins, int exact_out, int64_t count,
                                int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                                const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* given, char* msg, int64_t len)
{
    std::vector<cfmm::PathSegInfo> segs;
    for (int64_t s = 0; s < nseg; ++s) segs.push_back({kind[s], m[s], n_coins[s]});
    return cfmm::check_paths(exact_out ? "cfmm_quote_path_out" : "cfmm_quote_path", exact_out != 0, segs.data(), nseg, count, max_hops,
                             n_hops, hop_seg, hop_row, hop_coin_in, hop_coin_out, given, msg, (size_t)len);
}

namespace {

// A market of three segments -- product (5 pools), UniV3 (3), weighted with 4 coins (7) -- and a valid batch of 6 paths,
// max_hops 4, n_hops = 1 + p % 4, hop k of path p on segment (p + k) % 3; the slots a path does not use hold garbage that no
// check may look at.
struct Batch {
    static constexpr int64_t count = 6;
    static constexpr int32_t H = 4;
    std::vector<cfmm::PathSegInfo> segs{{0, 5, 2}, {2, 3, 2}, {3, 7, 4}};
    std::vector<int32_t> n_hops, seg, ci, co;
    std::vector<int64_t> row;
    std::vector<double> amt;
    Batch() : n_hops(count), seg(H * count, -77), ci(H * count, 99), co(H * count, 99), row(H * count, 1 << 30), amt(count)
    {
        for (int64_t p = 0; p < count; ++p) {
            n_hops[p] = 1 + (int)(p % H);
            amt[p] = 0.5 * (double)p;   // path 0 tenders exactly 0, which is valid
            for (int k = 0; k < n_hops[p]; ++k) {
                const int64_t at = k * count + p;
                seg[at] = (int32_t)((p + k) % 3);
                row[at] = (p + 2 * k) % segs[seg[at]].m;
                ci[at] = (int32_t)((p + k) % segs[seg[at]].n_coins);
                co[at] = (ci[at] + 1) % segs[seg[at]].n_coins;
            }
        }
    }
    int check(bool exact_out, char* msg, size_t len, int32_t max_hops = H, int64_t n = count) const
    {
        return cfmm::check_paths(exact_out ? "cfmm_quote_path_out" : "cfmm_quote_path", exact_out, segs.data(), (int64_t)segs.size(), n,
                                 max_hops, n_hops.data(), seg.data(), row.data(), ci.data(), co.data(), amt.data(), msg, len);
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
extern "C" int path_checks_host_cases()
{
    int bad = 0;
    char msg[256];
    const int E = CFMM_ERR_INVALID_ARG;
    for (int dir = 0; dir < 2; ++dir) {
        const bool out = dir != 0;
        const char* who = out ? "cfmm_quote_path_out:" : "cfmm_quote_path:";
        {
            Batch b;
            msg[0] = 0;
            bad += expect("valid batch", b.check(out, msg, sizeof msg), msg, CFMM_OK, nullptr);
            bad += expect("valid batch leaves the message alone", msg[0], msg, 0, nullptr);
            bad += expect("count 0", b.check(out, msg, sizeof msg, Batch::H, 0), msg, CFMM_OK, nullptr);
        }
        { Batch b; bad += expect("count < 0", b.check(out, msg, sizeof msg, Batch::H, -1), msg, E, "count must be >= 0"); }
        { Batch b; bad += expect("max_hops 0", b.check(out, msg, sizeof msg, 0), msg, E, "max_hops must be 1 .. 8"); }
        { Batch b; bad += expect("max_hops 9", b.check(out, msg, sizeof msg, 9), msg, E, "max_hops must be 1 .. 8"); }
        { Batch b; b.n_hops[4] = 0; bad += expect("n_hops 0", b.check(out, msg, sizeof msg), msg, E, "path 4: n_hops 0"); }
        { Batch b; b.n_hops[2] = 5; bad += expect("n_hops 5 of 4", b.check(out, msg, sizeof msg), msg, E, "path 2: n_hops 5"); }
        { Batch b; b.seg[2 * 6 + 3] = 3; bad += expect("segment", b.check(out, msg, sizeof msg), msg, E, "path 3, hop 2: segment 3 out of range"); }
        { Batch b; b.seg[0 * 6 + 5] = -1; bad += expect("segment < 0", b.check(out, msg, sizeof msg), msg, E, "path 5, hop 0: segment -1"); }
        { Batch b; b.row[1 * 6 + 1] = b.segs[b.seg[1 * 6 + 1]].m; bad += expect("row", b.check(out, msg, sizeof msg), msg, E, "path 1, hop 1: row"); }
        { Batch b; b.row[3 * 6 + 3] = -1; bad += expect("row < 0", b.check(out, msg, sizeof msg), msg, E, "path 3, hop 3: row -1"); }
        { Batch b; b.ci[1 * 6 + 2] = 2; b.seg[1 * 6 + 2] = 0; b.row[1 * 6 + 2] = 0;
          bad += expect("coin_in", b.check(out, msg, sizeof msg), msg, E, "path 2, hop 1: coin_in 2 out of range (pool has 2 coins)"); }
        { Batch b; b.co[0 * 6 + 0] = -1; bad += expect("coin_out", b.check(out, msg, sizeof msg), msg, E, "path 0, hop 0: coin_out -1"); }
        { Batch b; b.co[2 * 6 + 2] = b.ci[2 * 6 + 2]; bad += expect("same coins", b.check(out, msg, sizeof msg), msg, E, "path 2, hop 2: coin_in and coin_out are both"); }
        // the given amount enters at hop 0 (exact input) or at the path's last hop (exact output): path 3 has 4 hops
        { Batch b; b.amt[3] = -1.0; bad += expect("negative amount", b.check(out, msg, sizeof msg), msg, E, out ? "path 3, hop 3: amount_out" : "path 3, hop 0: amount_in"); }
        { Batch b; b.amt[1] = std::numeric_limits<double>::quiet_NaN(); bad += expect("NaN amount", b.check(out, msg, sizeof msg), msg, E, out ? "path 1, hop 1: amount_out" : "path 1, hop 0: amount_in"); }
        { Batch b; b.amt[5] = std::numeric_limits<double>::infinity(); bad += expect("inf amount", b.check(out, msg, sizeof msg), msg, E, "path 5, hop"); }
        { Batch b; b.amt[5] = -1.0; b.row[0 * 6 + 2] = -3; bad += expect("the first bad path is named", b.check(out, msg, sizeof msg), msg, E, "path 2, hop 0"); }
        { Batch b; b.seg[1 * 6 + 5] = 7; bad += expect("every message starts with the entry", b.check(out, msg, sizeof msg), msg, E, who); }
        {   // null arrays with count > 0
            Batch b;
            const int rc = cfmm::check_paths("cfmm_quote_path", false, b.segs.data(), 3, 6, 4, b.n_hops.data(), b.seg.data(), b.row.data(), b.ci.data(),
                                             nullptr, b.amt.data(), msg, sizeof msg);
            bad += expect("null hop_coin_out", rc, msg, E, "null path array");
        }
    }
    return bad;
}

#ifdef PATH_CHECKS_HOST_MAIN
int main()
{
    const int bad = path_checks_host_cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("PATH_CHECKS_HOST_OK\n");
    return 0;
}
#endif
