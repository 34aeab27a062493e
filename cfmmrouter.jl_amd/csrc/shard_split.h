// shard_split.h -- internal: how a multi-device parent splits a segment's pools, and a call's queries, over its shards.
// No HIP, no context.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace cfmm {

// shard d of nd holds rows [lo, hi) of a segment of m pools: contiguous blocks in device order, the first m % nd one longer
inline void shard_range(int64_t m, int d, int nd, int64_t& lo, int64_t& hi)
{
    const int64_t base = m / nd, rem = m % nd;
    lo = d * base + std::min<int64_t>(d, rem);
    hi = lo + base + (d < rem ? 1 : 0);
}

// the queries of one shard IN THE CALLER'S ORDER (the swaps depend on it): their positions in the call, their rows in the shard
struct ShardBucket {
    std::vector<int64_t> where, rows;
};

// one bucket per shard for `count` queries on rows idx[q] (null: query q is row q), every row in [0, m): one pass, a binary
// search on the blocks' ends per query
inline std::vector<ShardBucket> split_by_shard(int64_t m, int nd, int64_t count, const int64_t* idx)
{
    std::vector<int64_t> first((size_t)nd), end((size_t)nd);
    for (int d = 0; d < nd; ++d) shard_range(m, d, nd, first[(size_t)d], end[(size_t)d]);
    std::vector<ShardBucket> buckets((size_t)nd);
    for (int64_t q = 0; q < count; ++q) {
        const int64_t row = idx ? idx[q] : q;
        const size_t d = (size_t)(std::upper_bound(end.begin(), end.end(), row) - end.begin());   // first shard whose end > row
        buckets[d].where.push_back(q);
        buckets[d].rows.push_back(row - first[d]);
    }
    return buckets;
}

// a per-query column of the call as the bucket's shard takes it (src null: no column, an empty vector), and the way back
template <class T>
std::vector<T> gather(const std::vector<int64_t>& where, const T* src)
{
    std::vector<T> v(src ? where.size() : 0);
    for (size_t j = 0; j < v.size(); ++j) v[j] = src[where[j]];
    return v;
}
template <class T>
void scatter(const std::vector<int64_t>& where, const T* from, T* to)
{
    for (size_t j = 0; j < where.size(); ++j) to[where[j]] = from[j];
}

} // namespace cfmm
