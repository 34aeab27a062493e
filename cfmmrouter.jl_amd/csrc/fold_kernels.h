// fold_kernels.h -- what turns a sweep's partial rows into its result: the row fold (alone, or fused with the all-reduce
// of a sharded run) and the large-market gather.
#pragma once

#include "granule.h"
#include "sweep.h"

namespace cfmm {

// ---------------------------------------------------------------------------------------------
// Row fold: out[j] = sum over rows of partials[row][j]  (src/router.jl:81-83, :98-100 summed over blocks)
// ---------------------------------------------------------------------------------------------
// One block owns kReduceCols adjacent columns (64 B = half a 128-byte line of every row; rows are 128-byte aligned,
// SweepArgs::row_pitch).  lane = (row-lane r,
// column c): a wavefront holds 8 row-lanes x 8 columns.  Each lane sums its rows in increasing
// order (kBatch independent loads in flight), the row-lanes of a wavefront are folded by a fixed
// shuffle tree, the wavefronts by a fixed-order LDS pass: bit-reproducible for a fixed geometry.
//
// Block -> column group.  The two column groups of one 128-byte line are folded by two blocks; blocks are dealt round-robin
// to the 8 XCDs (block b runs on XCD b % 8, each with its own L2), so with "column group = block index" every line of the
// partial rows was fetched from the fabric TWICE, by two different L2s (round 4: 1491 KiB per fold for 526 KB of rows,
// together with rows that were not line-aligned).  Here the pair of groups {2p, 2p+1} belongs to blocks b = x + 8·(2j) and
// x + 8·(2j+1) with p = x + 8j: same XCD, consecutive deals -- the second request of a line is served by that XCD's L2
// (or merged with the first in flight).  Grid = 16·ceil(pairs / 8) blocks; a block beyond the last group returns.
// Placement is only a performance assumption: any placement computes the same result.
__device__ __forceinline__ int fold_colblock(int b)
{
    const int x = b & 7, q = b >> 3;
    return 2 * (x + 8 * (q >> 1)) + (q & 1);
}
static int fold_grid(int n1)
{
    const int groups = (n1 + kReduceCols - 1) / kReduceCols, pairs = (groups + 1) / 2;
    return 16 * ((pairs + 7) / 8);
}

__device__ __forceinline__ double fold_columns(const double* __restrict__ partials, int rows, int n1, int pitch, int colblock, double* red)
{
    constexpr int kRowLanes = kFoldBlock / kReduceCols;
    constexpr int kWaves = kFoldBlock / 64;
    constexpr int kBatch = 4;
    const int c = threadIdx.x % kReduceCols;
    const int r = threadIdx.x / kReduceCols;
    const int col = colblock * kReduceCols + c;
    double s = 0.0;
    if (col < n1) {
        const double* p = partials + col;
        int row = r;
        for (; row + (kBatch - 1) * kRowLanes < rows; row += kBatch * kRowLanes) {
            double x[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) x[b] = p[(size_t)(row + b * kRowLanes) * pitch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) s += x[b];
        }
        for (; row < rows; row += kRowLanes) s += p[(size_t)row * pitch];
    }
#pragma unroll
    for (int off = 32; off >= kReduceCols; off >>= 1) s += __shfl_down(s, off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < kReduceCols) red[wave * kReduceCols + lane] = s;
    __syncthreads();
    double tsum = 0.0;
    if (threadIdx.x < kReduceCols) {
        tsum = red[c];
        for (int k = 1; k < kWaves; ++k) tsum += red[k * kReduceCols + c];
    }
    return tsum;   // valid in threads [0, kReduceCols) with col < n1
}

// Tail of a fold block: its (up to) kReduceCols outputs go to `out` (plain stores, device consumers) or -- host.gran
// set -- to mapped host memory as SELF-VALIDATING granules {tag, 32 bits of the double} (two per column): the block's 8
// columns leave as 16 granules = 128 contiguous, 128-byte aligned bytes written by ONE store instruction (lane 2c + h
// carries half h of column c): two full 64-byte lines on the PCIe side -- a line written in pieces costs a
// read-modify-write per piece at the host's memory controller (measured: 2x slower evaluations).  Columns past n1
// travel as zeros so that the last block writes full lines too.  The host re-reads the granules until all carry the
// tag: no drain of the output stores, no ticket, no flag word.  Wavefront 0 only; tsum valid in lanes [0, kReduceCols).
__device__ __forceinline__ void fold_finish(double tsum, bool ok, int n1, int colblock, double* out, HostOut host)
{
    const int tid = threadIdx.x;
    if (tid >= 64) return;
    const int col = colblock * kReduceCols + tid;
    if (host.gran) {
        const double val = (tid < kReduceCols && col < n1) ? (ok ? tsum : __builtin_nan("")) : 0.0;
        const long long bits = __shfl(__double_as_longlong(val), (tid >> 1) & (kReduceCols - 1), 64);
        if (tid < 2 * kReduceCols) {
            __hip_atomic_store(host.gran + 2 * (size_t)colblock * kReduceCols + tid,
                               granule_of_bits(host.tag, (unsigned long long)bits, tid & 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (tid < kReduceCols && col < n1) {
        out[col] = ok ? tsum : __builtin_nan("");
    }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void reduce_partials(const double* __restrict__ partials, int rows, int n1, int pitch,
                                                         double* __restrict__ out, HostOut host, ArmWord arm)
{
    __shared__ double red[(BLOCK / 64) * kReduceCols];
    const int colblock = fold_colblock((int)blockIdx.x);
    if (colblock * kReduceCols >= n1) return;             // (block-uniform) padding of the grid to whole XCD deals
    // the fold of a pre-armed evaluation that was cancelled (or never got its prices) has nothing to publish; the
    // word cannot change between the threads' loads: the host moves on only after this launch's outputs
    if (arm.word && __hip_atomic_load(arm.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != arm.seq) return;
    const double tsum = fold_columns(partials, rows, n1, pitch, colblock, red);
    fold_finish(tsum, true, n1, colblock, out, host);
}

// Fold + all-reduce in one launch (sharded runs, see sweep.h).  The exchange uses self-validating
// 8-byte granules {tag = sequence number, 32 bits of payload} (MI355X_MICROARCH.md, hand-off form R2:
// "the data IS the flag"): each column travels as two granules (low / high half of the double), each
// written by ONE aligned 8-byte system-scope store, so there is no separate flag, no store drain and
// no second hop -- a reader simply re-reads a peer's granules (system-scope loads, which bypass the
// caches) until both carry this evaluation's tag.  This rank's own columns never leave registers.
// Double buffering by sequence parity: a rank rewrites gran[parity] for seq+2 only after its seq+1
// launch, which waited for every peer's seq+1 granules, i.e. for every peer's seq launch -- the one
// that read gran[parity] -- to have completed.  Waits are bounded by wall-clock time (NaN output).
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void reduce_gather(const double* __restrict__ partials, int rows, int n1, int pitch,
                                                       double* __restrict__ out, PeerSet ps)
{
    __shared__ double red[(BLOCK / 64) * kReduceCols];
    const int colblock = fold_colblock((int)blockIdx.x);
    if (colblock * kReduceCols >= n1) return;             // (block-uniform) padding of the grid to whole XCD deals
    // a cancelled pre-armed evaluation is cancelled on EVERY rank (the ranks run the same solver in lockstep):
    // nobody publishes, nobody waits, and the sequence number is reused by the next launch
    if (ps.arm.word && __hip_atomic_load(ps.arm.word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != ps.arm.seq) return;
    const double tsum = fold_columns(partials, rows, n1, pitch, colblock, red);
    const int tid = threadIdx.x;
    if (tid >= 64) return;                                // the exchange is wavefront 0's business
    const int parity = (int)(ps.seq & 1ull);
    // (the store and the peers' check below stay written out: through granule.h's granule / granule_join this kernel's
    // assembly changes, profiles/host_owners_digest.txt)
    const unsigned long long tag = granule_tag(ps.seq) << 32;
    const int col = colblock * kReduceCols + tid;
    if (tid < kReduceCols && col < n1 && ps.world > 1) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(tsum);
        unsigned long long* g = ps.gran[ps.rank] + 2 * ((long long)parity * ps.count + col);
        __hip_atomic_store(g, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(g + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // lane = (peer slot q, column c): 8 peers x 8 columns per pass, two passes cover kMaxPeers = 16
    const int q = tid / kReduceCols, c = tid % kReduceCols;
    const int colc = colblock * kReduceCols + c;
    const double own = __shfl(tsum, c, 64);
    double x[2] = {0.0, 0.0};
    bool ok = true;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int p = q + 8 * pass;
        if (p >= ps.world || colc >= n1) continue;
        if (p == ps.rank) { x[pass] = own; continue; }
        const unsigned long long* g = ps.gran[p] + 2 * ((long long)parity * ps.count + colc);
        const long long t0 = (long long)wall_clock64();
        for (;;) {
            const unsigned long long a = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long b = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((a & 0xffffffff00000000ull) == tag && (b & 0xffffffff00000000ull) == tag) {
                x[pass] = __longlong_as_double((long long)((a & 0xffffffffull) | (b << 32)));
                break;
            }
            if ((long long)wall_clock64() - t0 > ps.timeout_ticks) { ok = false; break; }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    ok = __all(ok);
    double s = 0.0;                                       // rank order on every rank: bit-identical results
    for (int p = 0; p < ps.world; ++p) s += __shfl(p < 8 ? x[0] : x[1], (p & 7) * kReduceCols + c, 64);
    fold_finish(s, ok, n1, colblock, out, ps.host);
}

// Large-market Ψ (see sweep_body<..., GBINS = true>).  entries[] lists, token by token, the flat
// indices 2·pool + side of the flows that belong to the token; it is cut into chunks of at most
// kGatherChunk entries so that hub tokens (a numeraire with 10⁵ pools) are spread over many
// wavefronts.  One wavefront per chunk: lane-strided partial sums, then a fixed shuffle tree.
__global__ __launch_bounds__(256) void gather_chunks(const int2* __restrict__ chunks, const int* __restrict__ entries,
                                                     const double* __restrict__ flow, double* __restrict__ chunk_sums,
                                                     int n_chunks)
{
    // 16 lanes per chunk (4 chunks per wavefront): a typical token has a few dozen incident
    // pools, so a full wavefront per chunk would idle most lanes and be latency-bound
    constexpr int kGroup = 16;
    const int chunk = (blockIdx.x * 256 + threadIdx.x) / kGroup, lane = threadIdx.x % kGroup;
    double s = 0.0;
    if (chunk < n_chunks) {
        const int2 ch = chunks[chunk];
        for (int e = ch.x + lane; e < ch.y; e += kGroup) s += flow[entries[e]];
    }
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kGroup);
    if (lane == 0 && chunk < n_chunks) chunk_sums[chunk] = s;
}

// out[t] = sum of token t's chunk sums, in chunk order (t < n); the block after the last token
// block folds the dual-scalar column of the partial rows into out[n] (lane-strided, fixed tree).
__global__ __launch_bounds__(256) void token_fold(const int* __restrict__ tok_chunk_off,
                                                  const double* __restrict__ chunk_sums, double* __restrict__ out, int n,
                                                  const double* __restrict__ acc_rows, int rows)
{
    const int token_blocks = (n + 255) / 256;
    if ((int)blockIdx.x < token_blocks) {
        const int t = blockIdx.x * 256 + threadIdx.x;
        if (t >= n) return;
        double s = 0.0;
        for (int c = tok_chunk_off[t]; c < tok_chunk_off[t + 1]; ++c) s += chunk_sums[c];
        out[t] = s;
        return;
    }
    __shared__ double wsum[4];
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) s += acc_rows[r];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[n] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

} // namespace cfmm
