// swap_order_waves.h -- internal, host only, no HIP: swap_path_waves.h's planner generalised from a path to a GROUP of paths,
// for cfmm_swap_order (abi_swap_order.cpp).  The orders are applied in the caller's order; the kernel runs eight lanes per
// order and no two orders of a launch may touch one pool.  Every pool (segment, row) carries the next wave it is free in (0 at
// the start); order g's wave number is the maximum of that over ALL pools of ALL its paths, and afterwards each of those
// pools is free from that wave + 1 on.  An order that turns out not to be applied (a refusing hop, a missed limit) still holds
// its pools for its wave: the host cannot know in advance.
// What follows from the rule: all paths of an order sit in one wave; inside a wave no two orders share a pool; for every pool
// the orders that name it have strictly increasing wave numbers in the caller's order; a batch of pool-disjoint orders is one
// wave; the numbering is minimal.  With one path per order it is swap_path_wave_numbers' numbering.
// tests/native/swap_order_host.cpp builds this for the CPU.
#pragma once

#include "swap_path_waves.h"

namespace cfmm {

// wave[g] for every order; order g owns the paths order_first[g] .. order_first[g+1] - 1 of hop-major arrays for n_paths paths
// (hop k of path p at k*n_paths + p; slots at k >= n_hops[p] are not looked at).  Returns the number of waves.
inline int64_t swap_order_wave_numbers(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops,
                                       const int32_t* hop_seg, const int64_t* hop_row, int64_t* wave, PathPoolTable* reuse = nullptr)
{
    size_t hops = 0;
    for (int64_t p = 0; p < n_paths; ++p) hops += n_hops[p] > 0 ? (size_t)n_hops[p] : 0;
    PathPoolTable own;
    PathPoolTable& table = reuse ? *reuse : own;
    table.reset(hops);
    int64_t waves = 0;
    for (int64_t g = 0; g < count; ++g) {
        int64_t w = 0;
        for (int64_t p = order_first[g]; p < order_first[g + 1]; ++p)
            for (int k = 0; k < n_hops[p]; ++k) w = std::max(w, table.free_from(hop_seg[(int64_t)k * n_paths + p], hop_row[(int64_t)k * n_paths + p]));
        for (int64_t p = order_first[g]; p < order_first[g + 1]; ++p)
            for (int k = 0; k < n_hops[p]; ++k) table.free_from(hop_seg[(int64_t)k * n_paths + p], hop_row[(int64_t)k * n_paths + p]) = w + 1;
        wave[g] = w;
        waves = std::max(waves, w + 1);
    }
    return waves;
}

// The launch order of the ORDERS, as SwapPathPlan states it for paths: perm[j] = the order at position j, wave after wave and
// in the caller's order within a wave; wave w is the positions wave_off[w] .. wave_off[w + 1].
inline SwapPathPlan swap_order_plan(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                    const int64_t* hop_row, PathPoolTable* reuse = nullptr)
{
    SwapPathPlan p;
    std::vector<int64_t> wave((size_t)count);
    const int64_t waves = swap_order_wave_numbers(count, order_first, n_paths, n_hops, hop_seg, hop_row, wave.data(), reuse);
    p.wave_off.assign((size_t)waves + 1, 0);
    for (int64_t g = 0; g < count; ++g) ++p.wave_off[(size_t)wave[(size_t)g] + 1];
    for (int64_t w = 0; w < waves; ++w) p.wave_off[(size_t)w + 1] += p.wave_off[(size_t)w];
    p.perm.resize((size_t)count);
    std::vector<int64_t> next(p.wave_off.begin(), p.wave_off.end() - 1);   // the next free position of each wave
    for (int64_t g = 0; g < count; ++g) p.perm[(size_t)next[(size_t)wave[(size_t)g]]++] = g;   // (a counting sort: stable)
    return p;
}

} // namespace cfmm
