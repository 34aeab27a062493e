// swap_path_waves.h -- internal, host only, no HIP: how cfmm_swap_path orders a batch of paths that share pools.  The paths
// are applied in query order; the kernel runs one lane per path and no two lanes may touch one pool.  So the batch is cut
// into WAVES, swap_waves.h's idea with a set of pools per query instead of one row: every pool (segment, row) carries the
// next wave it is free in (0 at the start); path p's wave number is the maximum of that over its pools, and afterwards each
// of its pools is free from that wave + 1 on.  A path that turns out not to be applied (a refused hop, a missed limit)
// still occupies its pools in its wave: the host cannot know in advance.
// What follows from the rule: inside a wave no two paths share a pool; for every pool the paths that name it have strictly
// increasing wave numbers in query order; a batch of pool-disjoint paths -- the common case -- is one wave; and the
// numbering is minimal, each path sits in the smallest wave that keeps the second property.
// THE planner below (swap_wave_numbers / swap_wave_plan) states the rule for OWNERS, groups of paths that are applied all or
// nothing: an owner's wave is the maximum over all pools of all its paths.  A batch of paths is the case of one path per
// owner, without an order_first array (swap_path_wave_numbers / swap_path_plan); cfmm_swap_order's orders are the general
// case (swap_order_waves.h).
// tests/native/swap_path_host.cpp builds this for the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cfmm {

// pool (segment, row) -> the next wave it is free in.  Open addressing with linear probing over one flat array of twice the
// hops of the batch: host memory proportional to count x max_hops, like everything else of the feature.  (A node-based map
// spent more than a microsecond per hop on a batch of a million paths.)  Sixteen neighbouring rows of a segment hash to
// sixteen neighbouring slots, so a dense batch walks the array instead of missing the cache at every hop; the object is kept
// between calls (cfmm_swap_path: SwapPathScratch) so that its pages are touched once.
class PathPoolTable {
    struct Slot {
        int64_t row;
        int64_t free_from;
        int32_t seg;
        int32_t used;
    };
    std::vector<Slot> slots_;

    size_t home(int32_t seg, int64_t row) const
    {
        uint64_t h = (uint64_t)(row >> 4) * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)seg;   // (splitmix64's finaliser)
        h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
        h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
        h ^= h >> 31;
        const size_t at = (size_t)(((unsigned __int128)h * slots_.size()) >> 64) + (size_t)(row & 15);   // [0, size) without a division
        return at < slots_.size() ? at : at - slots_.size();
    }

public:
    // empty, with room for `hops` distinct pools
    void reset(size_t hops)
    {
        slots_.resize(2 * hops + 16);
        std::fill(slots_.begin(), slots_.end(), Slot{0, 0, 0, 0});
    }
    // the pool's entry, created free from wave 0
    int64_t& free_from(int32_t seg, int64_t row)
    {
        size_t i = home(seg, row);
        while (slots_[i].used && !(slots_[i].seg == seg && slots_[i].row == row)) i = i + 1 == slots_.size() ? 0 : i + 1;
        if (!slots_[i].used) slots_[i] = Slot{row, 0, seg, 1};
        return slots_[i].free_from;
    }
};

// wave[g] for every owner; owner g has the paths order_first[g] .. order_first[g+1] - 1 (order_first null: path g alone, so
// count == n_paths) of hop-major arrays for n_paths paths (hop k of path p at k*n_paths + p; slots at k >= n_hops[p] are not
// looked at).  Returns the number of waves.
inline int64_t swap_wave_numbers(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                 const int64_t* hop_row, int64_t* wave, PathPoolTable* reuse = nullptr)
{
    size_t hops = 0;
    for (int64_t p = 0; p < n_paths; ++p) hops += n_hops[p] > 0 ? (size_t)n_hops[p] : 0;
    PathPoolTable own;
    PathPoolTable& table = reuse ? *reuse : own;
    table.reset(hops);
    int64_t waves = 0;
    for (int64_t g = 0; g < count; ++g) {
        const int64_t p0 = order_first ? order_first[g] : g, p1 = order_first ? order_first[g + 1] : g + 1;
        int64_t w = 0;
        for (int64_t p = p0; p < p1; ++p)
            for (int k = 0; k < n_hops[p]; ++k) w = std::max(w, table.free_from(hop_seg[(int64_t)k * n_paths + p], hop_row[(int64_t)k * n_paths + p]));
        for (int64_t p = p0; p < p1; ++p)
            for (int k = 0; k < n_hops[p]; ++k) table.free_from(hop_seg[(int64_t)k * n_paths + p], hop_row[(int64_t)k * n_paths + p]) = w + 1;
        wave[g] = w;
        waves = std::max(waves, w + 1);
    }
    return waves;
}

// The launch order: perm[j] = the owner at position j, wave after wave and in the caller's order within a wave (a counting
// sort by wave number, stable); wave w is the positions wave_off[w] .. wave_off[w + 1].
struct SwapPathPlan {
    std::vector<int64_t> perm, wave_off;
};
inline SwapPathPlan swap_wave_plan(int64_t count, const int64_t* order_first, int64_t n_paths, const int32_t* n_hops, const int32_t* hop_seg,
                                   const int64_t* hop_row, PathPoolTable* reuse = nullptr)
{
    SwapPathPlan p;
    std::vector<int64_t> wave((size_t)count);
    const int64_t waves = swap_wave_numbers(count, order_first, n_paths, n_hops, hop_seg, hop_row, wave.data(), reuse);
    p.wave_off.assign((size_t)waves + 1, 0);
    for (int64_t g = 0; g < count; ++g) ++p.wave_off[(size_t)wave[(size_t)g] + 1];
    for (int64_t w = 0; w < waves; ++w) p.wave_off[(size_t)w + 1] += p.wave_off[(size_t)w];
    p.perm.resize((size_t)count);
    std::vector<int64_t> next(p.wave_off.begin(), p.wave_off.end() - 1);   // the next free position of each wave
    for (int64_t g = 0; g < count; ++g) p.perm[(size_t)next[(size_t)wave[(size_t)g]]++] = g;
    return p;
}

// a batch of paths: one path per owner
inline int64_t swap_path_wave_numbers(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, int64_t* wave,
                                      PathPoolTable* reuse = nullptr)
{
    return swap_wave_numbers(count, nullptr, count, n_hops, hop_seg, hop_row, wave, reuse);
}
inline SwapPathPlan swap_path_plan(int64_t count, const int32_t* n_hops, const int32_t* hop_seg, const int64_t* hop_row, PathPoolTable* reuse = nullptr)
{
    return swap_wave_plan(count, nullptr, count, n_hops, hop_seg, hop_row, reuse);
}

} // namespace cfmm
