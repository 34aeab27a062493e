// swap_order_waves.h -- internal, host only, no HIP: the wave planner of swap_path_waves.h as cfmm_swap_order
// (abi_swap_order.cpp) names it -- the owners are ORDERS, groups of 1 .. 8 paths.  The orders are applied in the caller's
// order; the kernel runs eight lanes per order and no two orders of a launch may touch one pool.  Order g's wave number is the
// maximum of "free from" over ALL pools of ALL its paths, and afterwards each of those pools is free from that wave + 1 on.
// An order that turns out not to be applied (a refusing hop, a missed limit) still holds its pools for its wave: the host
// cannot know in advance.
// What follows from the rule: all paths of an order sit in one wave; inside a wave no two orders share a pool; for every pool
// the orders that name it have strictly increasing wave numbers in the caller's order; a batch of pool-disjoint orders is one
// wave; the numbering is minimal.  With one path per order it is swap_path_wave_numbers' numbering: both are one text.
// tests/native/swap_order_host.cpp builds this for the CPU.
#pragma once

#include "swap_path_waves.h"

namespace cfmm {

// wave[g] for every order; order g owns the paths order_first[g] .. order_first[g+1] - 1.  Returns the number of waves.
inline int64_t swap_order_wave_numbers(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops,
                                       const int32_t* hop_seg, const int64_t* hop_row, int64_t* wave, PathPoolTable* reuse = nullptr)
{
    return swap_wave_numbers(count, order_first, n_paths, n_hops, hop_seg, hop_row, wave, reuse);
}
// the launch order of the ORDERS (SwapPathPlan)
inline SwapPathPlan swap_order_plan(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                    const int64_t* hop_row, PathPoolTable* reuse = nullptr)
{
    return swap_wave_plan(count, order_first, n_paths, n_hops, hop_seg, hop_row, reuse);
}

} // namespace cfmm
