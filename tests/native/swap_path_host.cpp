// swap_path_host.cpp -- TEST-ONLY host build of csrc/swap_path_waves.h and csrc/swap_path_checks.h, the HIP-free parts of
// cfmm_swap_path: the wave numbering of paths that share pools and the checks beyond path_checks.h.  Two uses
// (tests/test_swap_path_cpu.py): built as a shared object and loaded with ctypes (one call of each function on the caller's
// arrays; swap_path_host_cases: the case list below), and built with -DSWAP_PATH_HOST_MAIN under the address and
// undefined-behaviour sanitizers as a stand-alone program that runs the same case list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/swap_path_checks.h"
#include "../../cfmmrouter.jl_amd/csrc/swap_path_waves.h"

extern "C" int64_t swap_path_host_waves(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, int64_t* wave)
{
    return cfmm::swap_path_wave_numbers(count, n_hops, hop_seg, hop_row, wave);
}

// perm [count], wave_off [count + 1] (the first waves + 1 entries are written); returns the number of waves
extern "C" int64_t swap_path_host_plan(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, int64_t* perm,
                                       int64_t* wave_off)
{
    const cfmm::SwapPathPlan p = cfmm::swap_path_plan(count, n_hops, hop_seg, hop_row);
    std::memcpy(perm, p.perm.data(), p.perm.size() * sizeof(int64_t));
    std::memcpy(wave_off, p.wave_off.data(), p.wave_off.size() * sizeof(int64_t));
    return (int64_t)p.wave_off.size() - 1;
}

extern "C" int swap_path_host_check(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row,
                                    const double* min_amount_out, char* msg, int64_t len)
{
    return cfmm::check_swap_paths("cfmm_swap_path", count, n_hops, hop_seg, hop_row, min_amount_out, msg, (size_t)len);
}

namespace {

// paths given as lists of pools {segment, row}; the hop arrays are built hop-major with garbage in the unused slots
struct Batch {
    int64_t count;
    int32_t H = 0;
    std::vector<int32_t> n_hops, seg;
    std::vector<int64_t> row;
    explicit Batch(const std::vector<std::vector<std::pair<int32_t, int64_t>>>& paths) : count((int64_t)paths.size())
    {
        for (const auto& p : paths) H = std::max<int32_t>(H, (int32_t)p.size());
        n_hops.resize((size_t)count);
        seg.assign((size_t)(H * count), -77);
        row.assign((size_t)(H * count), (int64_t)1 << 40);
        for (int64_t p = 0; p < count; ++p) {
            n_hops[(size_t)p] = (int32_t)paths[(size_t)p].size();
            for (size_t k = 0; k < paths[(size_t)p].size(); ++k) {
                seg[k * (size_t)count + (size_t)p] = paths[(size_t)p][k].first;
                row[k * (size_t)count + (size_t)p] = paths[(size_t)p][k].second;
            }
        }
    }
    std::vector<int64_t> waves(int64_t* n = nullptr) const
    {
        std::vector<int64_t> w((size_t)count, -1);
        const int64_t got = cfmm::swap_path_wave_numbers(count, n_hops.data(), seg.data(), row.data(), w.data());
        if (n) *n = got;
        return w;
    }
    int check(const double* lim, char* msg, size_t len) const
    {
        return cfmm::check_swap_paths("cfmm_swap_path", count, n_hops.data(), seg.data(), row.data(), lim, msg, len);
    }
};

int expect(const char* what, bool ok)
{
    if (!ok) std::printf("FAILED %s\n", what);
    return ok ? 0 : 1;
}

int expect_msg(const char* what, int rc, const char* msg, int want_rc, const char* want_text)
{
    const bool ok = rc == want_rc && (want_text == nullptr || std::strstr(msg, want_text) != nullptr);
    if (!ok) std::printf("FAILED %s: rc %d, message '%s' (wanted rc %d, '%s')\n", what, rc, msg, want_rc, want_text ? want_text : "");
    return ok ? 0 : 1;
}

} // namespace

// the case list; returns the number of cases that did not behave
extern "C" int swap_path_host_cases()
{
    int bad = 0;
    const std::pair<int32_t, int64_t> A{0, 5}, B{1, 5}, C{1, 6}, D{2, 0};   // (A and B: the same row of different segments)
    int64_t n = 0;
    {   // the worked case: {A,B} {B,C} {D} {C,A} -> 0 1 0 2
        const Batch b({{A, B}, {B, C}, {D}, {C, A}});
        bad += expect("worked case", b.waves(&n) == std::vector<int64_t>{0, 1, 0, 2} && n == 3);
        const cfmm::SwapPathPlan p = cfmm::swap_path_plan(b.count, b.n_hops.data(), b.seg.data(), b.row.data());
        bad += expect("worked case, launch order", p.perm == std::vector<int64_t>{0, 2, 1, 3} && p.wave_off == std::vector<int64_t>{0, 2, 3, 4});
    }
    {   // pool-disjoint paths are one wave, in query order
        const Batch b({{A}, {B, C}, {D}});
        bad += expect("disjoint", b.waves(&n) == std::vector<int64_t>{0, 0, 0} && n == 1);
        const cfmm::SwapPathPlan p = cfmm::swap_path_plan(b.count, b.n_hops.data(), b.seg.data(), b.row.data());
        bad += expect("disjoint, launch order", p.perm == std::vector<int64_t>{0, 1, 2} && p.wave_off == std::vector<int64_t>{0, 3});
    }
    {   // a chain: every path shares a pool with its predecessor -> one wave each
        const Batch b({{A, B}, {B, C}, {C, D}, {D, A}});
        bad += expect("chain", b.waves(&n) == std::vector<int64_t>{0, 1, 2, 3} && n == 4);
    }
    {   // the same pool three times, an unrelated path in between: it joins wave 0
        const Batch b({{A}, {A}, {D}, {A}});
        bad += expect("repeats", b.waves(&n) == std::vector<int64_t>{0, 1, 0, 2} && n == 3);
    }
    {   // a late path that touches only pools freed early sits as low as its pools allow, not behind the batch's last wave
        const Batch b({{A}, {A}, {A}, {B}, {B, C}});
        bad += expect("minimal", b.waves(&n) == std::vector<int64_t>{0, 1, 2, 0, 1} && n == 3);
    }
    {
        const Batch b({});
        bad += expect("empty", b.waves(&n).empty() && n == 0);
        const cfmm::SwapPathPlan p = cfmm::swap_path_plan(0, nullptr, nullptr, nullptr);
        bad += expect("empty plan", p.perm.empty() && p.wave_off == std::vector<int64_t>{0});
    }
    // the checks
    char msg[256];
    const int E = CFMM_ERR_INVALID_ARG;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    {
        const Batch b({{A, B}, {B, C, D}, {D}});
        const double lim[3] = {0.0, 1.5, 1e300};
        msg[0] = 0;
        bad += expect_msg("valid, no limits", b.check(nullptr, msg, sizeof msg), msg, CFMM_OK, nullptr);
        bad += expect_msg("valid, limits", b.check(lim, msg, sizeof msg), msg, CFMM_OK, nullptr);
        bad += expect("a valid batch leaves the message alone", msg[0] == 0);
        for (const double x : {-1.0, nan, inf, -inf}) {
            double l2[3] = {0.0, x, 2.0};
            bad += expect_msg("bad limit", b.check(l2, msg, sizeof msg), msg, E, "cfmm_swap_path: path 1, hop 2: min_amount_out must be finite and >= 0");
        }
        const double l3[3] = {-0.0, 0.0, 0.0};
        bad += expect_msg("-0.0 is a limit", b.check(l3, msg, sizeof msg), msg, CFMM_OK, nullptr);
    }
    {
        const Batch b({{A, B}, {B, C, D, C}, {D, D}});
        bad += expect_msg("repeated pool", b.check(nullptr, msg, sizeof msg), msg, E, "cfmm_swap_path: path 1, hops 1 and 3: row 6 of segment 1 appears twice");
    }
    {
        const Batch b({{A, B}, {A, D}, {D, C, D}});
        const double lim[3] = {0.0, -1.0, 0.0};
        bad += expect_msg("the first bad path is named", b.check(lim, msg, sizeof msg), msg, E, "path 1, hop 1: min_amount_out");
        bad += expect_msg("repeated pool, first and last hop", b.check(nullptr, msg, sizeof msg), msg, E, "path 2, hops 0 and 2: row 0 of segment 2");
    }
    {   // the same row in different segments is two pools
        const Batch b({{A, B}});
        bad += expect_msg("same row, other segment", b.check(nullptr, msg, sizeof msg), msg, CFMM_OK, nullptr);
    }
    return bad;
}

#ifdef SWAP_PATH_HOST_MAIN
int main()
{
    const int bad = swap_path_host_cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("SWAP_PATH_HOST_OK\n");
    return 0;
}
#endif
