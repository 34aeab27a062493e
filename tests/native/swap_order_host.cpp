// swap_order_host.cpp -- TEST-ONLY host build of csrc/swap_order_waves.h, the HIP-free planner of cfmm_swap_order: the wave
// numbering of ORDERS (groups of paths) that share pools.  Two uses (tests/test_swap_order_cpu.py): built as a shared object
// and loaded with ctypes (one call of each function on the caller's arrays; swap_order_host_cases: the case list below), and
// built with -DSWAP_ORDER_HOST_MAIN under the address and undefined-behaviour sanitizers as a stand-alone program that runs
// the same case list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cfmmrouter.jl_amd/csrc/swap_order_waves.h"

extern "C" int64_t swap_order_host_waves(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                         const int64_t* hop_row, int64_t* wave)
{
    return cfmm::swap_order_wave_numbers(count, order_first, n_paths, n_hops, hop_seg, hop_row, wave);
}

// perm [count], wave_off [count + 1] (the first waves + 1 entries are written); returns the number of waves
extern "C" int64_t swap_order_host_plan(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                        const int64_t* hop_row, int64_t* perm, int64_t* wave_off)
{
    const cfmm::SwapPathPlan p = cfmm::swap_order_plan(count, order_first, n_paths, n_hops, hop_seg, hop_row);
    std::memcpy(perm, p.perm.data(), p.perm.size() * sizeof(int64_t));
    std::memcpy(wave_off, p.wave_off.data(), p.wave_off.size() * sizeof(int64_t));
    return (int64_t)p.wave_off.size() - 1;
}

// the path planner on the same arrays, for "one path per order is swap_path_plan"
extern "C" int64_t swap_order_host_path_plan(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, int64_t* perm,
                                             int64_t* wave_off)
{
    const cfmm::SwapPathPlan p = cfmm::swap_path_plan(count, n_hops, hop_seg, hop_row);
    std::memcpy(perm, p.perm.data(), p.perm.size() * sizeof(int64_t));
    std::memcpy(wave_off, p.wave_off.data(), p.wave_off.size() * sizeof(int64_t));
    return (int64_t)p.wave_off.size() - 1;
}

namespace {

using Pool = std::pair<int32_t, int64_t>;
using Path = std::vector<Pool>;
using Order = std::vector<Path>;

// orders given as lists of paths, paths as lists of pools {segment, row}; the hop arrays are built hop-major with garbage in
// the unused slots
struct Batch {
    int64_t count, n_paths = 0;
    int32_t H = 1;
    std::vector<int64_t> first, row;
    std::vector<int32_t> n_hops, seg;
    explicit Batch(const std::vector<Order>& orders) : count((int64_t)orders.size())
    {
        first.push_back(0);
        std::vector<Path> flat;
        for (const Order& o : orders) {
            for (const Path& p : o) {
                flat.push_back(p);
                H = std::max<int32_t>(H, (int32_t)p.size());
            }
            first.push_back((int64_t)flat.size());
        }
        n_paths = (int64_t)flat.size();
        n_hops.resize((size_t)n_paths);
        seg.assign((size_t)(H * n_paths), -77);
        row.assign((size_t)(H * n_paths), (int64_t)1 << 40);
        for (int64_t p = 0; p < n_paths; ++p) {
            n_hops[(size_t)p] = (int32_t)flat[(size_t)p].size();
            for (size_t k = 0; k < flat[(size_t)p].size(); ++k) {
                seg[k * (size_t)n_paths + (size_t)p] = flat[(size_t)p][k].first;
                row[k * (size_t)n_paths + (size_t)p] = flat[(size_t)p][k].second;
            }
        }
    }
    std::vector<int64_t> waves(int64_t* n = nullptr) const
    {
        std::vector<int64_t> w((size_t)count, -1);
        const int64_t got = cfmm::swap_order_wave_numbers(count, first.data(), n_paths, n_hops.data(), seg.data(), row.data(), w.data());
        if (n) *n = got;
        return w;
    }
    cfmm::SwapPathPlan plan(cfmm::PathPoolTable* reuse = nullptr) const
    {
        return cfmm::swap_order_plan(count, first.data(), n_paths, n_hops.data(), seg.data(), row.data(), reuse);
    }
};

int expect(const char* what, bool ok)
{
    if (!ok) std::printf("FAILED %s\n", what);
    return ok ? 0 : 1;
}

} // namespace

// the case list; returns the number of cases that did not behave
extern "C" int swap_order_host_cases()
{
    int bad = 0;
    const Pool A{0, 5}, B{1, 5}, C{1, 6}, D{2, 0}, E{2, 1}, F{0, 6};   // (A and B: the same row of different segments)
    int64_t n = 0;
    {   // the worked case: order 1 shares B with order 0 through its SECOND path, order 3 shares C with order 1 and A with 0
        const Batch b({{{A}, {B}}, {{C}, {D, B}}, {{E}}, {{C, A}, {F}}});
        bad += expect("worked case", b.waves(&n) == std::vector<int64_t>{0, 1, 0, 2} && n == 3);
        const cfmm::SwapPathPlan p = b.plan();
        bad += expect("worked case, launch order", p.perm == std::vector<int64_t>{0, 2, 1, 3} && p.wave_off == std::vector<int64_t>{0, 2, 3, 4});
    }
    {   // pool-disjoint orders are one wave, in the caller's order
        const Batch b({{{A}, {B, C}}, {{D}}, {{E}, {F}}});
        bad += expect("disjoint", b.waves(&n) == std::vector<int64_t>{0, 0, 0} && n == 1);
        const cfmm::SwapPathPlan p = b.plan();
        bad += expect("disjoint, launch order", p.perm == std::vector<int64_t>{0, 1, 2} && p.wave_off == std::vector<int64_t>{0, 3});
    }
    {   // a chain: every order shares a pool with its predecessor -> one wave each
        const Batch b({{{A}, {B}}, {{B}, {C}}, {{C}, {D}}, {{D}, {A}}});
        bad += expect("chain", b.waves(&n) == std::vector<int64_t>{0, 1, 2, 3} && n == 4);
    }
    {   // the maximum runs over ALL paths of the order: the last path decides
        const Batch b({{{A}}, {{A}}, {{A}}, {{B}, {C}, {D, A}}, {{B}}});
        bad += expect("every path counts", b.waves(&n) == std::vector<int64_t>{0, 1, 2, 3, 4} && n == 5);
    }
    {   // a late order that touches only pools freed early sits as low as its pools allow
        const Batch b({{{A}}, {{A}}, {{A}}, {{B}}, {{B}, {C}}});
        bad += expect("minimal", b.waves(&n) == std::vector<int64_t>{0, 1, 2, 0, 1} && n == 3);
    }
    {   // the planner's table may be kept between calls
        cfmm::PathPoolTable keep;
        const Batch b1({{{A}, {B}}, {{B}}}), b2({{{A}}, {{C}}});
        const cfmm::SwapPathPlan p1 = b1.plan(&keep), p2 = b2.plan(&keep);
        bad += expect("reused table", p1.wave_off == std::vector<int64_t>{0, 1, 2} && p2.wave_off == std::vector<int64_t>{0, 2});
    }
    {
        const Batch b({});
        bad += expect("empty", b.waves(&n).empty() && n == 0);
        const cfmm::SwapPathPlan p = b.plan();
        bad += expect("empty plan", p.perm.empty() && p.wave_off == std::vector<int64_t>{0});
    }
    return bad;
}

#ifdef SWAP_ORDER_HOST_MAIN
int main()
{
    const int bad = swap_order_host_cases();
    if (bad) {
        std::printf("%d cases failed\n", bad);
        return 1;
    }
    std::printf("SWAP_ORDER_HOST_OK\n");
    return 0;
}
#endif
