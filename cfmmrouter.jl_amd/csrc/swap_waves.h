// swap_waves.h -- internal, host only, no HIP: how cfmm_swap orders a batch that names a row more than once.  The swaps are
// applied in query order; the kernel runs one lane per swap and no two lanes may touch one pool.  So the batch is cut into
// WAVES: swap q's wave number is the number of earlier queries on the same row, wave w holds every query of wave number w, and
// the waves are launched one after the other in stream order.  Within a wave the rows are distinct by construction and
// sorted ascending (ties cannot occur), so a dense batch stays coalesced.  A batch of distinct rows -- the common case -- is
// one wave.  tests/native/swap_host.cpp builds this for the CPU.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace cfmm {

// wave[q] = the number of queries before q on the same row; idx == null: query q is row q (all zero).  Returns the number of waves.
inline int64_t swap_wave_numbers(int64_t count, const int64_t* idx, int64_t* wave)
{
    if (!idx) {
        std::fill(wave, wave + count, (int64_t)0);
        return count > 0 ? 1 : 0;
    }
    std::vector<std::pair<int64_t, int64_t>> a((size_t)count);
    for (int64_t q = 0; q < count; ++q) a[(size_t)q] = {idx[q], q};
    std::sort(a.begin(), a.end());   // by row, then by position in the batch
    int64_t waves = 0;
    for (size_t k = 0, w = 0; k < a.size(); ++k) {
        w = k > 0 && a[k].first == a[k - 1].first ? w + 1 : 0;
        wave[a[k].second] = (int64_t)w;
        waves = std::max(waves, (int64_t)w + 1);
    }
    return waves;
}

// The launch order: perm[j] = the query at position j, wave after wave and rows ascending within a wave; wave w is the
// positions wave_off[w] .. wave_off[w + 1].
struct SwapPlan {
    std::vector<int64_t> perm, wave_off;
};
inline SwapPlan swap_plan(int64_t count, const int64_t* idx)
{
    SwapPlan p;
    std::vector<int64_t> wave((size_t)count);
    const int64_t waves = swap_wave_numbers(count, idx, wave.data());
    p.perm.resize((size_t)count);
    for (int64_t q = 0; q < count; ++q) p.perm[(size_t)q] = q;
    if (idx)
        std::sort(p.perm.begin(), p.perm.end(), [&](int64_t x, int64_t y) {
            return wave[(size_t)x] != wave[(size_t)y] ? wave[(size_t)x] < wave[(size_t)y] : idx[x] < idx[y];
        });
    p.wave_off.assign((size_t)waves + 1, 0);
    for (int64_t q = 0; q < count; ++q) ++p.wave_off[(size_t)wave[(size_t)q] + 1];
    for (int64_t w = 0; w < waves; ++w) p.wave_off[(size_t)w + 1] += p.wave_off[(size_t)w];
    return p;
}

} // namespace cfmm
