// sweep.h -- internal C++ interface between the C ABI (abi_*.cpp) and the gfx950 kernels
// (sweep_kernels.hip and the device headers it includes).  Not installed; the public surface is include/cfmm_amd.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace cfmm {

constexpr int kMidBlock = 512;       // 8 wavefronts: small markets (one tile per block) and fused multi-family launches
constexpr int kBigBlock = 1024;      // 16 wavefronts: single-family launches, few partial rows
constexpr int kFoldBlock = 512;      // reduce_partials / reduce_gather
constexpr int kResidentThreads = 2048 * 256; // one machine of resident threads (256 CUs x 2048)
constexpr int kReduceCols = 8;       // tokens per fold block (64 B = half a 128-byte line of each partial row; the two blocks that share
                                     // a line run on the SAME XCD, i.e. behind the same L2: fold_colblock in fold_kernels.h)
constexpr int kRowAlign = 16;        // partial rows are padded to a multiple of this many doubles (128 B)
constexpr int kMaxLdsTokens = 8192;  // up to here the prices + one bin copy fit the 160 KiB LDS of a CU;
                                     // larger markets pull Ψ per token (sweep_body<..., GBINS=true>)
constexpr int kGatherChunk = 512;    // incidence entries per wavefront in gather_chunks

// SoA-of-pairs pool stores, one struct per pool family.  All pointers are device pointers.
// Packed fee + token-index record (8 B instead of 16): tok = i1 | i2 << 16 (n_tokens <= 65536), gidx = index of
// the pool's fee in the launch's fee table (markets use a handful of fee tiers; the table, <= kMaxFeeTable distinct
// values per launch, is staged in LDS).  Segments whose fees do not fit keep the plain gamma / Ai arrays (pk == null).
struct PackedFeeTok {
    uint32_t tok;
    uint32_t gidx;
};
constexpr int kMaxFeeTable = 256;

// Window of the "fast" arithmetic (fast_arith.h, div_by / fast_sqrt): when every reserve, fee, liquidity and
// price of a launch lies in [2^-kFastExp, 2^kFastExp], the IEEE division / square-root sequences run without their
// range scaffolding (v_div_scale, v_div_fmas, v_div_fixup, ldexp pairs) and still return the correctly rounded bits.
constexpr int kFastExp = 150;

struct ProductPools {            // src/cfmms.jl:101-111
    const double2* R;            // [m] {R1, R2}
    const double* gamma;         // [m]
    const int2* Ai;              // [m] {i1, i2}, 0-based
    const PackedFeeTok* pk;      // [m] {tokens, fee-table index}: replaces Ai (and gamma) in the sweep (24 B per pool instead of
                                 //     32); null only in large-market mode (n_tokens > kMaxLdsTokens: plain arrays)
    int gbase;                   // this segment's first entry in the launch's fee table, or -1: no table (too many fee tiers,
                                 //     or option "pack" = 0): the fee comes from gamma[]
};
struct GeoMeanPools {            // src/cfmms.jl:152-165
    const double2* R;
    const double2* w;            // [m] {w1, w2}
    const double* gamma;
    const int2* Ai;
    const double* eta;           // [m] η = w1/w2                  prepared at upload
    const double2* Q;            // [m] {Q1, Q2}: the v-independent part of the two log-space exponents, prepared at
                                 //     upload: Q1 = log γ + log η + log R2 + η·log R1,  Q2 = η·(log γ + log R1 − log η) + log R2
    int reference_order;         // 1: evaluate with pow in the reference's operation order
    const PackedFeeTok* pk;      // see ProductPools (48 B per pool instead of 56)
    int gbase;
};
// One tick of a walk list (UniV3Ops::list_tick): everything find_arb_pos (src/cfmms.jl:321-337) needs for one prepared
// tick in ONE 64-byte line -- lanes walk different pools, so every tick visit is a scattered access; round 2 kept
// {k, s_in}, {δmax, s_out} and R_out in three arrays = three lines per visit.
struct alignas(64) TickRec {
    double2 ks;                  // {k, R_in + alpha_in}
    double2 dt;                  // {delta_max, R_out + beta_out}
    double rout;                 // R_out
    double thr;                  // this tick's drain threshold (the same value as UniV3Pools::thr[...]; 0: never / closing record): the
                                 // walk's 2^-40 band test needs it exactly where the record is already in registers
    double2 psum;                // {Σδ, Σλ} of the current tick and of every list tick BEFORE this one, all drained, summed in
                                 // walk order (UniV3Ops::solve_dir); every list is closed by a record that carries only this
};
struct UniV3Pools {              // src/cfmms.jl:226-245 as find_arb_pos constants (see UniV3Ops)
    const double2* pg;           // [m] {current_price, gamma}
    const int2* Ai;              // [m]
    const double2* cur_a;        // [m] current tick {k, R1+alpha}
    const double2* cur_b;        // [m] current tick {R2+beta, k/beta - (R1+alpha)}
    const double* cur_c;         // [m] current tick  k/alpha - (R2+beta)
    const double2* curR;         // [m] current tick {R1, R2}
    const int4* walk;            // [m] ticks beyond the current one: {up_begin, up_count, lo_begin, lo_count}
    const TickRec* ticks;        // [W] the walk lists: per pool the non-empty ticks above, then below, its current one, each
                                 //     list closed by one extra record (psum of the whole list)
    const double* thr;           // [W] per record: the largest price at which the walk drains that tick (0: never / closing record)
    const uint4* head;           // [2m] or null.  Round 5: the first FOUR drain thresholds of pool i's two walk lists ({up, down} =
                                 //     head[2i], head[2i+1]) as binary32 values rounded DOWN (bits; 0 = never drains, a NaN pattern =
                                 //     "not representable: ask the exact array"), read with the pool's other coalesced streams.  With
                                 //     lo = the float and hi = the next float up, lo <= T <= hi: price <= lo proves that the tick
                                 //     drains, price > hi proves that it does not, anything in between falls back to the exact scan
                                 //     of thr[] -- so the walk decisions are the exact ones, while four of five walking pools no longer
                                 //     touch thr[] (whose 128-byte lines were being fetched almost in full for 32 useful bytes each)
    int has_walk;                // 0: no pool of the segment has a tick beyond its current one (every BoundedProduct
                                 //    pool): the walk spans are not even loaded
    const double* cp;            // [m] current_price alone, read with pk instead of pg + Ai (packed records)
    const PackedFeeTok* pk;      // see ProductPools
    int gbase;
};

// N-coin pools, one launch per segment (sweep_ncoin): the weighted geometric-mean family (GeometricMean / Product,
// src/cfmms.jl:57-64; WeightedFamily) and the Curve (StableSwap) family, φ(R) = α·Σ R − β·Π R⁻¹ (Curve{T},
// src/cfmms.jl:66-70; CurveFamily, curve_pool.h).  Per-coin columns are COIN-MAJOR ([n_coins][m]: coin k of pool i at
// k·m + i), so the lanes of a wavefront (consecutive pools) load each column as one coalesced stream.
constexpr int kMaxCoins = 8;
struct NCoinPools {
    const double* R;             // [n_coins][m] reserves
    const double* q;             // [n_coins][m] the family's per-coin constant, prepared at upload and by update_ncoin:
                                 //     weighted log(R / w) (the v-independent part of s^λ = log(R·v/w)), Curve log R
    const int32_t* tok;          // [n_coins][m] token indices, 0-based
    const double2* glg;          // [m] {γ, log γ}
    const double* par;           // the family's own column: weighted [n_coins][m] weights (normalised to sum to 1 at
                                 //     upload), Curve [m] {α, log β}
    int n_coins;                 // 2 .. kMaxCoins, uniform over the segment
    double* Delta;               // [n_coins][m] trades of a materialising sweep (null otherwise)
    double* Lambda;
};

// How a fold launch hands {Ψ, acc} to the host (mapped pinned memory), if at all: gran != null -> the block's 8 columns
// leave as 16 SELF-VALIDATING 8-byte granules {tag, 32 bits of the double} (two per column) written by one store
// instruction = two full 64-byte lines; the host re-reads them until all carry the tag -- no drain of the output stores,
// no ticket, no flag word.  gran == null: plain stores to `out` (device consumers).
struct HostOut {
    unsigned long long* gran;    // [2 * ceil8(n1)] words in mapped host memory, or null
    unsigned long long tag;      // 1 .. 2^32 - 1 (0 = an empty buffer)
};
struct SweepArgs {
    const double* v;             // [n] device
    int n;                       // n_tokens
    int n_pad;                   // n rounded up to even (LDS row pitch)
    int v_shift;                 // 4: prices staged in LDS as {v, rcp_refined(v)} pairs (16 B per token: the fast arithmetic's
                                 //    divisions by a price); 3: the prices alone (markets too wide for the pairs)
    int need_logv;               // 1: also stage log v per token in LDS (launches with a log-space GeometricMean segment)
    const double* gtab;          // the launch's fee table (device), staged in LDS when gtab_n > 0
    int gtab_n;
    int copies;                  // private bin copies per block (1 or one per wavefront)
    unsigned long long* flags;   // sticky report word in mapped host memory (or null): kFlagWindow / kFlagGaveUp, set by a block
                                 //    that poisons its row (see sweep_tiles)
    int64_t m;                   // pools in this segment
    // Trade buffers of the segment (null when !materialize).  compact == 0: Delta[i] = {Δ₁, Δ₂}, Lambda[i] = {Λ₁, Λ₂}
    // (32 B written per pool).  compact == 1: at most one direction of a pool trades, so ONE 16-byte record goes
    // to Delta[i]:  {+Δ₁, Λ₂}  (direction 1 or no trade)  or  {−Δ₂, Λ₁}  (direction 2; the sign bit of the first
    // entry carries the direction, −0.0 included); any other pool -- both directions non-zero (γ > 1), NaN, or the tiny
    // negative / −0.0 values the reference's tick arithmetic yields on degenerate UniV3 boundaries -- writes the record
    // {0, −1} and its four values to Lambda[i] = {Δ₁, Δ₂}, Over[i] = {Λ₁, Λ₂}.  Lossless bit for bit; decoded by
    // cfmm_get_trades / expand_trades / update_two_coin.
    double2* Delta;
    double2* Lambda;
    double2* Over;
    int compact;
    double* partials;            // [grid][row_pitch] rows of this launch ([grid][1] with global bins)
    int row_pitch;               // doubles between two partial rows: n+1 rounded up to a multiple of 16 (128-byte rows: a fold block's
                                 //    64-byte column group never straddles a line; round 4's pitch of n+1 doubles shifted every row by
                                 //    8 bytes: 1491 KiB fetched for 526 KB of rows), 1 with global bins
    double2* gflow;              // null: LDS bins; else [m] {Λ₁−Δ₁, Λ₂−Δ₂} of this segment (large markets)
    int reverse;                 // 1: every lane walks its tiles last-to-first (alternates between consecutive sweeps, so a
                                 //    sweep starts on the pool data the previous one left in the XCD's L2)
    // Pre-armed launch (arm_word != null; cfmm_route): the kernel is enqueued BEFORE its price vector exists and every
    // block, after issuing its first pool loads and clearing its bins, waits until the host has written v into `v`
    // (fine-grained device memory, through the PCIe BAR) and then arm_seq into *arm_word -- the launch latency is
    // spent while the previous evaluation and the host solver run.  *arm_word == arm_seq | kArmCancel: the launch
    // is not needed (the blocks skip their pools, the fold returns without output).  Waits are bounded by
    // arm_timeout ticks of the 100 MHz wall clock; a block that gives up poisons the dual column with NaN.
    const unsigned long long* arm_word;
    unsigned long long arm_seq;
    long long arm_timeout;
    // Single-block launches (grid == 1: markets of up to kDirectPools pools, one family): the block's row IS the result, so
    // it goes straight to `direct_out` (device consumers) or -- direct_host.gran set -- to the host as granules, and NO fold
    // launch follows: one kernel per evaluation instead of two (the reference's own benchmark grid, benchmark/scaling.jl:8-38,
    // has six of its ten market sizes in this range, where an evaluation is launch latency and nothing else).
    int nt_stores;               // 1: trade records leave through non-temporal stores (HBM-resident markets); 0: write-through
    int direct;
    double* direct_out;          // [n + 1] {Ψ, acc}
    HostOut direct_host;
};
constexpr int kDirectPools = 2048;   // two tiles of a 1024-thread block
constexpr unsigned long long kArmCancel = 1ull << 63;
constexpr unsigned long long kFlagWindow = 1;   // a fast kernel staged a price outside [2^-kFastExp, 2^kFastExp]: rows poisoned
constexpr unsigned long long kFlagGaveUp = 2;   // a pre-armed launch gave up waiting for its price vector: rows poisoned

// One launch over up to kMaxMulti segments (sweep_multi).
constexpr int kMaxMulti = 4;
union AnyPools {
    ProductPools p;
    GeoMeanPools g;
    UniV3Pools u;
    NCoinPools n;                // (sweep_ncoin launches only: never in a SegRec)
};
static_assert(sizeof(AnyPools) == sizeof(UniV3Pools), "SegRec's layout is the widest two-coin family's");

// The launch-invariant descriptor of a sweep_kernel / sweep_multi launch.  Everything a launch of a given geometry reads
// that does NOT change from one evaluation to the next -- pool pointers, segment sizes, the block -> segment map, trade and
// row buffers, the fee table, the LDS geometry -- lives in DEVICE memory: built on the host by build_sweep_desc
// (launch_plan.h) when the geometry, an option or an array it points to changes, uploaded once, and then read by every
// launch through the scalar cache.  Nothing rewrites it between launches, so from the second sweep on its lines CAN be
// served by each XCD's L2 (expected, not measured: what is measured is the entry's length); the kernel
// arguments proper (SweepLaunch) are one 128-byte line.  Before, a fused launch carried 0x390
// bytes of arguments (eight lines, written afresh and therefore cache-cold on every XCD for every launch) and walked
// them in nine dependent waits -- xcd_map, pattern[] / rank[], seg_w[], seg[sidx]... -- before its first pool load.
//
// BlockRec, indexed by blockIdx.x: the block's segment, the first pool of its tile 0 (lane 0), the distance between two of
// its tiles, and how many tiles a lane walks: lane t has `full + (t < tail)` -- no division on the device.  The records
// restate the maps the kernels used to compute (sweep_multi's two forms, bid / gridDim for a segment's own launch): the
// same block sweeps the same pools in the same order and writes the same row.
struct BlockRec {
    int64_t first;               // pool of lane 0 in the block's tile 0
    int64_t stride;              // pools between two consecutive tiles of the block (blocks of the segment x block size)
    int32_t full;                // tiles every lane of the block has
    int32_t tail;                // lanes of one more, partial tile (0: none)
    int32_t row;                 // partial row the block writes
    int16_t seg;                 // segment of the launch
    int16_t kind;                // its CFMM_KIND_*
};
static_assert(sizeof(BlockRec) == 32, "four block records per 128-byte line");
// One segment of the launch: the pool streams first (what the first tile's loads need), then what the epilogues need
struct SegRec {
    AnyPools pools;
    int64_t m;
    double2* Delta;              // the segment's rows of the trade buffers (always set; read by materialising kernels only)
    double2* Lambda;
    double2* Over;
    double2* gflow;              // large-market mode: the segment's rows of the flow array, else null
};
struct SweepDesc {
    int n, n_pad, v_shift, need_logv;           // SweepArgs' fields of the same names
    const double* gtab;
    int gtab_n, copies;
    unsigned long long* flags;
    double* partials;            // row 0 of this launch
    int row_pitch, compact, nt_stores, direct;
    int nseg, grid;              // segments, block records
    SegRec seg[kMaxMulti];
    // BlockRec[grid] follows at kSweepDescHead (128-byte aligned)
};
constexpr size_t kSweepDescHead = (sizeof(SweepDesc) + 127) / 128 * 128;
inline size_t sweep_desc_bytes(int grid) { return kSweepDescHead + ((size_t)grid * sizeof(BlockRec) + 127) / 128 * 128; }
// What differs between two launches of the same geometry: the kernels' arguments, inside the first 128 bytes of the
// kernarg segment.  The kernels take the leading scalars as four parameters of their own -- what gfx950 hands over in
// SGPRs before the first instruction (kernarg preload: csrc/Makefile KFLAGS) -- and the tail as one by-value struct that
// is read from the segment where it is first used.
struct SweepTail {               // SweepArgs::arm_* / direct_out / direct_host
    const unsigned long long* arm_word;
    unsigned long long arm_seq;
    long long arm_timeout;
    double* direct_out;
    HostOut direct_host;
};
struct SweepLaunch {
    const SweepDesc* desc;       // device
    const double* v;             // [n] device
    int reverse;                 // SweepArgs::reverse
    int n;                       // n_tokens (== desc->n)
    SweepTail tail;
};
// (the Makefile's KFLAGS preload five arguments: the folds' partials, rows, n1, pitch, out; of the sweeps' arguments the four
// scalars -- a by-value struct is not preloaded)
constexpr int kSweepScalars = 4;
static_assert(offsetof(SweepLaunch, tail) == 24 && sizeof(SweepLaunch) <= 128,
              "the per-launch arguments are one line of the kernarg segment, the preloaded ones its first 6 dwords");

struct LaunchCfg {
    int block;                   // kMidBlock or kBigBlock
    int grid;
    size_t lds_bytes;
    int arith = 0;               // the kernel's arithmetic (sweep_core.h, FASTK): 0 = the compiler's full-range sequences,
                                 // 1 = fast (every pool constant of the launch and -- the host KNOWS -- every price inside the
                                 // kFastExp window), 2 = auto (pool constants inside the window, prices unknown to the host:
                                 // device-pointer sweeps; every block picks the loop from the prices it stages)
    bool lean = false;           // the lean form of the kernel (launch_plan.h lean_launch said so); a family, block or arithmetic
                                 // without one: hipErrorInvalidDeviceFunction, like every other missing kernel
    hipEvent_t ev_start = nullptr; // both set: the launch is timed by the command processor
    hipEvent_t ev_stop = nullptr;  // (hipExtLaunchKernel), i.e. the kernel's own execution span
};

// A two-coin segment's own launch (sweep_kernel) from its descriptor.  `kind` picks the kernel family: ProductTwoCoin,
// GeometricMeanTwoCoin (reference_order picks the pow-based form), UniV3 (the threshold-head kernel when `heads` is set
// outside large-market mode), Solidly-style stable pairs (CFMM_KIND_SOLIDLY, φ = x³y + xy³: ProductTwoCoin's pool layout,
// full-range arithmetic).  Large-market mode (gbins) runs kMidBlock threads on the full-range arithmetic.  A combination of
// family, arithmetic, block and mode that has no kernel (sweep_kernels.hip, the kernel table) returns
// hipErrorInvalidDeviceFunction.
hipError_t launch_sweep(int kind, bool reference_order, bool heads, bool gbins, const SweepLaunch& la, const LaunchCfg& c,
                        bool materialize, hipStream_t s);
// An N-coin segment's launch (sweep_ncoin; CFMM_KIND_WEIGHTED / CFMM_KIND_CURVE): kMidBlock threads, full-range arithmetic,
// never single-block direct; there is no large-market kernel (gbins set: hipErrorInvalidDeviceFunction); a.Delta / a.Lambda / a.Over / a.gflow are unused, the trades go to pools.Delta /
// pools.Lambda.
hipError_t launch_ncoin(int kind, const NCoinPools& pools, const SweepArgs& a, bool gbins, const LaunchCfg& c, bool materialize,
                        hipStream_t s);
// R <- (R + γΔ) − Λ per coin, in place, then q <- the family's constant for the new R (par: unchanged)
hipError_t launch_update_ncoin(int kind, double* R, double* q, const double* par, const double2* glg, const double* Delta,
                               const double* Lambda, int n_coins, int64_t m, hipStream_t s);

// Several segments in one launch (sweep_multi) from the launch's descriptor; block b writes partial row b.
hipError_t launch_multi(bool gbins, const SweepLaunch& la, const LaunchCfg& c, bool materialize, hipStream_t s);

// Large markets: chunk_sums[c] = sum of flow[entries[chunks[c].x .. chunks[c].y)], then
// out[t] = sum of chunk_sums[tok_chunk_off[t] .. tok_chunk_off[t+1]) for t < n and
// out[n] = sum of acc_rows[0 .. rows) (the dual-scalar column of the partial rows).
hipError_t launch_gather(const int2* chunks, const int* entries, const double* flow, double* chunk_sums, int n_chunks,
                         const int* tok_chunk_off, double* out, int n, const double* acc_rows, int rows, hipStream_t s);

struct ArmWord {                 // see SweepArgs::arm_word; {nullptr, 0} = not armed
    const unsigned long long* word;
    unsigned long long seq;
};
// rows of n1 doubles, `pitch` doubles apart (SweepArgs::row_pitch)
inline int row_pitch_of(int n1) { return (n1 + kRowAlign - 1) / kRowAlign * kRowAlign; }
// out[j] = sum over rows of partials[row][j], j in [0, n1); fixed summation order.
hipError_t launch_reduce(const double* partials, int rows, int n1, int pitch, double* out, hipStream_t s,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, HostOut host = HostOut{nullptr, 0},
                         ArmWord arm = ArmWord{nullptr, 0});

// Sharded runs (cfmm_set_peers): the row fold fused with the one-shot all-reduce over xGMI peer
// mappings (reduce_gather in fold_kernels.h): block b folds its kReduceCols columns, publishes
// them as self-validating granules in this rank's symmetric buffer and adds the same columns of
// every peer in rank order -- one launch, one hop on the critical path, no hand-off between the blocks of a rank.
constexpr int kMaxPeers = 16;
struct PeerSet {
    unsigned long long* gran[kMaxPeers];    // peer p's granules: [2][count][2] uint64 (see include/cfmm_amd.h)
    int world, rank;
    long long count;                        // n_tokens + 1
    unsigned long long seq;                 // 1, 2, ... identical on every rank
    long long timeout_ticks;                // wall_clock64() ticks (100 MHz) before a wait gives up (NaN output)
    HostOut host;                           // optional: the global {Ψ, acc} also travel to the host as granules
    ArmWord arm;                            // pre-armed evaluation: a cancelled launch publishes nothing
};
hipError_t launch_reduce_gather(const double* partials, int rows, int n1, int pitch, double* out, hipStream_t s,
                                const PeerSet& ps, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// R <- (R + gamma*Delta) - Lambda in place; GeometricMean (Q, eta non-null): Q <- the exponents' constants for the new R;
// *left_window <- 1 if a new reserve lies outside [2^-kFastExp, 2^kFastExp]
hipError_t launch_update_two_coin(double2* R, const double* gamma, const double2* Delta, const double2* Lambda,
                                  const double2* Over, int compact, double2* Q, const double* eta, int64_t m, int* left_window,
                                  hipStream_t s);
// Sparse pool-state updates (cfmm_pools_set_*, abi_update.cpp): one launch scatters the host-prepared records of `count` pools
// into every affected column of ONE segment.  The staging buffer (device-visible, 8-byte words) holds the columns one after
// the other, column c as rows x width words from word `begin`; row j of a column goes to row idx[j] of the column's device
// array (dst, `width` words per row) -- or, for a column appended to an array (UniV3 walk records and thresholds at the
// tail), to row dense_base + j.  Coin-major columns ([n_coins][m]) are n_coins columns of width 1.  The host has checked
// every idx and the tail's capacity.
constexpr int kMaxScatterCols = 2 * kMaxCoins + 2;
struct ScatterCol {
    unsigned long long* dst;
    long long begin;             // first word of the column in the staging buffer (columns in ascending order; gaps allowed)
    long long rows;
    long long dense_base;        // >= 0: the column's rows are dense_base + j, not idx[j]
    int width;                   // 8-byte words per row
};
struct ScatterArgs {
    const unsigned long long* stage;
    const long long* idx;        // [count] rows within the segment, distinct (staging)
    long long total;             // words of all columns together
    int ncols;
    ScatterCol col[kMaxScatterCols];
};
hipError_t launch_scatter_records(const ScatterArgs& a, hipStream_t s);
// Compaction of a UniV3 segment's tick records (update_kernels.h compact_walks): pool i's walk.y + walk.w + 2 records move from
// old_ticks + old_walk[i].x to ticks + new_walk[i].x; thr[e] <- record e's thr, thr[tail .. tail + 4) <- 0, walk_out <- new_walk.
// new_walk may be device-visible host memory; the other arrays are device arrays, old and new distinct.  e0, e1: both set =
// the launch is timed by the command processor.
hipError_t launch_compact_walks(const int4* old_walk, const int4* new_walk, int4* walk_out, const TickRec* old_ticks, TickRec* ticks,
                                double* thr, int64_t m, int64_t tail, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// compact trade records -> full {Δ₁, Δ₂} / {Λ₁, Λ₂} arrays (cfmm_trades_dev, cfmm_get_trades*)
hipError_t launch_expand_trades(const double2* rec, const double2* ovA, const double2* ovB, double2* Delta, double2* Lambda,
                                int64_t m, hipStream_t s);

// cfmm_select_trades (select_kernels.h, abi_trades.cpp): the rows of ONE segment that trade and are worth min_value, compacted
// in pool order by three launches.  The view of one call; all pointers are device pointers.
constexpr int kSelBlock = 256;        // pools per block of select_flag / select_emit: one lane per pool, 4 mask words per block
constexpr int kSelScanChunk = 1024;   // block counts the single block of select_scan folds per step
struct SelectArgs {
    int64_t m;                   // pools of the segment
    int n_coins;                 // doubles per output row: 2, or the ragged segment's coin count
    const double* v;             // [n_tokens] the prices the trades are valued at
    double min_value;
    // two-coin kinds: the segment's rows of the trade buffers (SweepArgs: plain or compact layout) and its tokens
    const double2* Delta;
    const double2* Lambda;
    const double2* Over;
    int compact;
    const PackedFeeTok* pk;      // the packed records, or null: Ai
    const int2* Ai;
    // ragged kinds: the coin-major columns ([n_coins][m], NCoinPools)
    const double* ncD;
    const double* ncL;
    const int32_t* nctok;
    // scratch
    unsigned long long* mask;    // [blocks][kSelBlock / 64] one bit per pool
    int* counts;                 // [blocks]
    long long* base;             // [blocks] exclusive prefix sums of counts
    // outputs (select_emit): the first `capacity` selected rows; each may be null
    long long capacity;
    long long* out_idx;          // [capacity] rows within the segment
    double* out_D;               // [capacity][n_coins]
    double* out_L;
    double* out_value;           // [capacity]
};
inline int64_t select_blocks(int64_t m) { return (m + kSelBlock - 1) / kSelBlock; }
// flag + count, then the scan, which stores the total to *total_host (device address of pinned host memory); `ragged` picks
// the instantiation.  ev: null, or three {start, stop} pairs for the three kernels (launch_select_emit takes ev[4], ev[5]).
hipError_t launch_select_count(const SelectArgs& a, bool ragged, long long* total_host, hipStream_t s, hipEvent_t* ev);
hipError_t launch_select_emit(const SelectArgs& a, bool ragged, hipStream_t s, hipEvent_t* ev);

// cfmm_quote / cfmm_quote_dev (quote_kernels.h, abi_quote.cpp): exact-input swap quotes of ONE segment, one lane per query.
// All pointers are device pointers; the pool streams are the segment's own arrays (nothing is uploaded or kept per pool).
constexpr int kQuoteBlock = 256;
struct QuoteArgs {
    int64_t count;               // queries
    int64_t m;                   // pools of the segment
    int n_coins;                 // 2, or the ragged segment's coin count
    const long long* idx;        // [count] rows within the segment, any order, repeats allowed; null: query q is row q
    const int32_t* coin_in;      // [count] positions in the pool's own coin order
    const int32_t* coin_out;     // [count], or null (two-coin kinds, UniV3): 1 − coin_in
    const double* amount_in;     // [count]
    double* amount_out;          // [count]; NaN for a query whose row, coins or amount are out of range (never read out of bounds)
    // two-coin kinds (Product, Solidly, GeometricMean): reserves, weights (GeometricMean only), fees
    const double2* R;
    const double2* w;
    const double* gamma;
};
// `kind` picks the instantiation; u: UniV3 segments, n: weighted / Curve segments (the other members unused).  e0, e1: both
// set = the launch is timed by the command processor.
hipError_t launch_quote(int kind, const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                        hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// cfmm_quote_out / cfmm_quote_out_dev: the inverse kernels (quote_out_kernel) on the same arguments -- `amount_in` is then the
// wanted output and `amount_out` receives the input to tender.
hipError_t launch_quote_out(int kind, const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                            hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_swap (swap_kernels.h, abi_swap.cpp): exact-input swaps that move the pools, one lane per swap of ONE WAVE -- queries whose
// rows are distinct (the host numbers the waves).  `q` is the wave's view as quote_kernel takes it; the members below are the
// segment's own arrays again, writable.  The n_coins kinds write through ncR / ncq (NCoinPools::R / ::q of the same launch).
struct SwapArgs {
    QuoteArgs q;
    double2* R;                  // two-coin kinds: [m] reserves
    double2* Q;                  // GeometricMean: [m] {Q1, Q2}
    const double* eta;           // GeometricMean: [m] η
    double* ncR;                 // weighted / Curve: [n_coins][m]
    double* ncq;
    double* price;               // UniV3: [count] the price each swap comes to rest at (the kernel changes no UniV3 state)
    int* left_window;            // <- 1 when a new reserve lies outside [2^-kFastExp, 2^kFastExp] (kinds with a fast arithmetic), or null
};
hipError_t launch_swap(int kind, const SwapArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0 = nullptr,
                       hipEvent_t e1 = nullptr);

// cfmm_swap_out (swap_out_kernels.h, abi_swap.cpp): exact-output swaps that move the pools, one lane per swap of one wave.
// `s` is swap_kernel's view with the roles of the two amounts exchanged as in quote_out_kernel: s.q.amount_in carries the
// wanted output, s.q.amount_out receives the input tendered.
constexpr int32_t kSwapApplied = 0, kSwapOverLimit = 1, kSwapRefused = 2, kSwapUnobtainable = 3;   // CFMM_SWAP_* (include/cfmm_amd.h)
struct SwapOutArgs {
    SwapArgs s;
    const double* max_in;        // [count], or null: no limit
    int32_t* status;             // [count], never null: kSwap*
};
hipError_t launch_swap_out(int kind, const SwapOutArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                           hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_quote_path / cfmm_quote_path_out (quote_path_kernels.h, abi_quote_path.cpp): an amount carried through a PATH of up
// to CFMM_MAX_PATH_HOPS pools of any segments in one launch, one lane per path.  The first kernels that read several segments
// of different kinds at once: the segments reach them as a TABLE in device memory (a market may have more segments than fit
// in kernel arguments), one PathSeg each -- the kind, the sizes and exactly the pointers quote_one<KIND> reads.  The table is
// rebuilt from the segments' `.get()` addresses and uploaded on EVERY call (abi_quote_path.cpp): it is never a cache.
struct PathSeg {
    int32_t kind;                // CFMM_KIND_*, or -1: a segment without pools (no hop can be valid on it; nothing is read)
    int32_t n_coins;             // 2, or the ragged segment's coin count
    int64_t m;                   // pools of the segment
    // two-coin kinds (QuoteArgs::R / w / gamma)
    const double2* R;
    const double2* w;
    const double* gamma;
    // UniV3: the seven members of UniV3Pools the quotes read
    const double2* pg;
    const double2* cur_a;
    const double2* cur_b;
    const double* cur_c;
    const double2* curR;
    const int4* walk;
    const TickRec* ticks;
    // weighted / Curve: the four members of NCoinPools the quotes read
    const double* nR;
    const double* nq;
    const double2* nglg;
    const double* npar;
};
struct PathArgs {
    int64_t count;               // paths
    int32_t max_hops;            // rows of the hop arrays, 1 .. CFMM_MAX_PATH_HOPS
    int32_t nseg;                // records of `segs`
    const PathSeg* segs;         // [nseg] device
    const int32_t* n_hops;       // [count]; outside 1 .. max_hops: the whole path is NaN and no hop is evaluated
    // hop-major: hop k of path p at k*count + p (neighbouring lanes read neighbouring words); slots at k >= n_hops[p] unread
    const int32_t* hop_seg;
    const long long* hop_row;
    const int32_t* hop_coin_in;
    const int32_t* hop_coin_out;
    const double* given;         // [count] amount_in (quote_path_kernel) / the wanted amount_out (quote_path_out_kernel)
    double* answer;              // [count]
    double* hops;                // [max_hops][count] or null: the amount leaving hop k / the amount to tender to hop k; NaN in
                                 // the unused slots
};
// exact_out picks quote_path_out_kernel.  e0, e1: both set = the launch is timed by the command processor.
hipError_t launch_quote_path(bool exact_out, const PathArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_size_path (size_path_kernels.h, abi_size_path.cpp): the input of a path that maximises its gain, one WAVEFRONT per
// path and one lane per trial size.  The paths are a PathArgs as cfmm_quote_path's kernel takes it -- p.given is
// max_amount_in, p.answer receives amount_in, p.hops is unused (null) -- plus the arrays of the search.
struct SizeArgs {
    PathArgs p;
    const double* value_in;      // [count], or null: 1.0
    const double* value_out;     // [count], or null: 1.0
    int32_t rounds;              // 1 .. CFMM_MAX_SIZE_ROUNDS
    double* amount_out;          // [count]
    double* gain;                // [count]
    int32_t* status;             // [count] CFMM_SIZED*
};
constexpr int kSizeBlock = 256;                                  // four wavefronts = four paths per block
constexpr int kSizeMaxBlocks = kResidentThreads / kSizeBlock;    // default of option "size_max_blocks": one machine of resident wavefronts
// max_blocks >= 1 caps the grid (the wavefronts stride over the paths).  e0, e1: both set = the launch is timed.
hipError_t launch_size_path(const SizeArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_split_paths (split_paths_kernels.h, abi_split_paths.cpp): an order's amount spread over its 1 .. 8 paths, one WAVEFRONT
// per order and one lane per grid point.  The paths are a PathArgs as cfmm_quote_path's kernel takes it -- p.count is n_paths,
// p.given is unused (null), p.answer receives path_amount_in, p.hops is unused (null) -- plus the orders.
struct SplitArgs {
    PathArgs p;
    int64_t orders;              // orders
    const long long* order_first; // [orders + 1]: order g owns the paths order_first[g] .. order_first[g+1] - 1
    const double* amount;        // [orders] the amount to spread
    int32_t rounds;              // 1 .. CFMM_MAX_SPLIT_ROUNDS
    double* path_out;            // [p.count] path_amount_out
    double* total;               // [orders]
    int32_t* status;             // [orders] CFMM_SPLIT_*
};
constexpr int kSplitBlock = 256;                                  // four wavefronts = four orders per block
constexpr int kSplitMaxBlocks = kResidentThreads / kSplitBlock;   // default of option "split_max_blocks": one machine of resident wavefronts
// max_blocks >= 1 caps the grid (the wavefronts stride over the orders).  e0, e1: both set = the launch is timed.
hipError_t launch_split_paths(const SplitArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// cfmm_split_paths_out (split_paths_out_kernels.h): the same arguments with the roles of the amounts exchanged, as PathArgs
// serves both quote directions -- amount carries the wanted output B, p.answer receives path_amount_out (the shares of B),
// path_out receives path_amount_in (what each share costs), total is total_in.  The same block, the same grid rule.
hipError_t launch_split_paths_out(const SplitArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_swap_path (swap_path_kernels.h, abi_swap_path.cpp): exact-input paths that MOVE their pools, all or nothing, one lane per
// path of ONE WAVE -- paths that share no pool (the host numbers the waves: swap_path_waves.h).  The kernel reads a table of
// its own: what PathSeg holds (the quotes' view, unchanged), the segment's arrays again as writable pointers, what
// swap_kernel takes besides them (GeometricMean's {Q1, Q2} and η) and the segment's window flag.  Rebuilt and uploaded per
// call, and again after a wave that moved UniV3 pools (their arrays may have been replaced), like the path table.
struct SwapPathSeg {
    PathSeg s;
    double2* R;                  // two-coin kinds: [m] reserves
    double2* Q;                  // GeometricMean: [m] {Q1, Q2}
    const double* eta;           // GeometricMean: [m] η
    double* nR;                  // weighted / Curve: [n_coins][m]
    double* nq;
    int* left_window;            // <- 1 when a new reserve of THIS segment lies outside [2^-kFastExp, 2^kFastExp] (kinds with a
                                 //    fast arithmetic), or null
    int64_t pad[2];
};
static_assert(sizeof(PathSeg) == 128 && sizeof(SwapPathSeg) == 192, "PathSeg stays one line; the swap table adds half of one");
constexpr int32_t kPathApplied = 0, kPathBelowLimit = 1, kPathRefused = 2;   // CFMM_PATH_* (include/cfmm_amd.h)
struct SwapPathArgs {
    int64_t count;               // paths of this wave
    int64_t stride;              // paths of the call: hop k of the wave's path p at k*stride + p of the arrays below, which
                                 // already point at the wave's first path
    int32_t max_hops;            // 1 .. CFMM_MAX_PATH_HOPS
    int32_t nseg;                // records of `segs`
    const SwapPathSeg* segs;     // [nseg] device
    const int32_t* n_hops;       // [count]
    const int32_t* hop_seg;      // hop-major, as PathArgs
    const long long* hop_row;
    const int32_t* hop_coin_in;
    const int32_t* hop_coin_out;
    const double* amount_in;     // [count]
    const double* min_out;       // [count], or null: no limit
    double* amount_out;          // [count]
    double* hops;                // [max_hops][stride], never null: the amount leaving hop k (pass 2 reads it back)
    double* price;               // [max_hops][stride]: the price a UniV3 hop comes to rest at (the kernel changes no UniV3 state)
    int32_t* status;             // [count] kPathApplied / kPathBelowLimit / kPathRefused
};
hipError_t launch_swap_path(const SwapPathArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// cfmm_swap_path_out (swap_path_out_kernel): the same arguments with the roles of the amounts exchanged, as PathArgs serves
// both quote directions -- amount_in carries the wanted output of the LAST hop, min_out the limit on the input (max_amount_in),
// amount_out receives the input to tender to the first hop, hops the amount TO TENDER to hop k, and status is one of kSwap*.
hipError_t launch_swap_path_out(const SwapPathArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_swap_order / cfmm_swap_order_out (swap_order_kernels.h, abi_swap_order.cpp): orders that MOVE their pools, each all or
// nothing across its 1 .. 8 paths, EIGHT LANES PER ORDER of ONE WAVE -- orders that share no pool (swap_order_waves.h).  The
// paths are a SwapPathArgs as swap_path_kernel takes it, for ALL paths of the call: p.count == p.stride == n_paths, the
// arrays point at the call's first path (order_first names paths by their position in them), p.min_out is unused (null),
// p.status receives path_status.  The orders' arrays point at the wave's first order.
constexpr int32_t kOrderApplied = 0, kOrderLimit = 1, kOrderRefused = 2, kOrderUnobtainable = 3;   // CFMM_ORDER_* (include/cfmm_amd_order.h)
constexpr int32_t kOrderPathHeld = 4;                                                              // CFMM_ORDER_PATH_HELD
struct SwapOrderArgs {
    SwapPathArgs p;
    int64_t orders;               // orders of this wave
    const long long* order_first; // [orders + 1]: order g owns the paths order_first[g] .. order_first[g+1] - 1
    const double* limit;          // [orders] min_total_out / max_total_in, or null: no limit
    double* total;                // [orders]
    int32_t* status;              // [orders] kOrder*
};
constexpr int kOrderBlock = 256;                                  // four wavefronts = 32 orders per block
constexpr int kOrderMaxBlocks = kResidentThreads / kOrderBlock;   // default of option "order_max_blocks": one machine of resident wavefronts
// max_blocks >= 1 caps the grid (the wavefronts stride over the wave's orders).  e0, e1: both set = the launch is timed.
hipError_t launch_swap_order(bool exact_out, const SwapOrderArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0 = nullptr,
                             hipEvent_t e1 = nullptr);

// cfmm_find_path (find_path_kernels.h, abi_find_path.cpp): the best walk of at most max_hops hops between two tokens, by
// layers -- one launch per layer with ONE LANE PER POOL of every segment.  The kernels read a table of their own: what
// PathSeg holds (the quotes' view, unchanged), the segment's token arrays (two-coin kinds and UniV3: the packed records, or
// the plain pairs in large-market mode, as SelectArgs; ragged kinds: the coin-major column) and where the segment starts in
// the two numberings the kernels use -- blocks of the per-pool launches, and pools of the whole market (the order of the
// tie-break).  Rebuilt and uploaded per call, like the path table.
constexpr int kFindBlock = 256;          // pools per block of the per-pool launches (a segment starts a new block)
constexpr int kFindLaneQueries = 64;     // queries one lane serves (one bit each of its reached mask); gridDim.y covers the rest
struct FindSeg {
    PathSeg s;
    const PackedFeeTok* pk;      // two-coin kinds, UniV3: {i1 | i2 << 16, .}, or null (large-market mode)
    const int2* Ai;              //   ... then the plain pairs
    const int32_t* tok;          // ragged kinds: [n_coins][m]; null otherwise
    int64_t first_tile;          // blocks of the segments before this one
    int64_t first_pool;          // pools of the segments before this one
    int64_t pad[3];
};
static_assert(sizeof(FindSeg) == 192, "the find table: a PathSeg and half a line");
struct FindArgs {
    int64_t count;               // queries of this chunk
    int64_t stride;              // queries of the call: hop k of the chunk's query q at k*stride + q of the hop arrays below
    int32_t max_hops;            // 1 .. CFMM_MAX_PATH_HOPS
    int32_t nseg;                // records of `segs`
    int32_t n_tokens;
    int32_t layer;               // find_relax / find_claim / find_advance: 1 .. max_hops
    int64_t tiles;               // blocks of kFindBlock pools that cover every segment's pools
    int32_t group;               // find_relax with the LDS copy: queries per grid row (1 .. kFindLaneQueries), 0: no LDS copy
    int32_t tiles_per_block;     //   ... and tiles one block folds into its copy before it touches global memory
    const FindSeg* segs;         // [nseg] device
    // all per-query arrays already point at the chunk's first query
    const int32_t* token_in;     // [count] 0-based
    const int32_t* token_out;
    const double* amount_in;
    unsigned long long* best;    // [max_hops + 1][count][n_tokens] the layers: a positive finite double's bits, 0 = unreached
    unsigned long long* edge;    // [max_hops][count] the claimed hop that ENDS layer k + 1, packed; all ones: none
    int32_t* h_star;             // [count] hops of the answer, 0: none
    int32_t* target;             // [count] the token the walk back stands at
    double* amount_out;          // [count]
    int32_t* n_hops;
    int32_t* status;             // CFMM_FOUND*
    int32_t* hop_seg;            // [max_hops][stride], -1 in the unused slots
    long long* hop_row;
    int32_t* hop_coin_in;
    int32_t* hop_coin_out;
};
// the LDS copy of find_relax: group x n_tokens words within this many bytes (four blocks of it fit a CU beside their registers)
constexpr int kFindLdsBytes = 32768;
inline int find_lds_group(int n_tokens) { const int g = kFindLdsBytes / 8 / (n_tokens < 1 ? 1 : n_tokens); return g > kFindLaneQueries ? kFindLaneQueries : g; }
// kFindOut*: cfmm_find_path_out, the same search run backwards from the wanted output (find_path_kernels.h).  FindArgs serves
// it with the roles of the amounts exchanged, as PathArgs serves both quote directions: amount_in carries the wanted
// amount_out, amount_out receives the amount to tender, best holds the layers of a MIN-search (all ones = unreached), edge[k]
// is hop k in path order and target is the token the forward walk stands at.
enum FindKernel { kFindInit, kFindRelax, kFindSelect, kFindClaim, kFindAdvance, kFindFinish,
                  kFindOutInit, kFindOutRelax, kFindOutSelect, kFindOutClaim, kFindOutAdvance, kFindOutFinish };
constexpr int kFindOutFirst = kFindOutInit;   // a kFindOut* value minus this is the exact-input kernel of the same role
// e0, e1: both set = the launch is timed by the command processor
hipError_t launch_find(FindKernel which, const FindArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_find_disjoint_paths (find_disjoint_kernels.h, abi_find_disjoint.cpp): round `round` of the successive search -- the four
// exact-input kernels that know the ban (kFindInit, kFindRelax, kFindClaim, kFindFinish; select and advance are launch_find's)
// take FindArgs UNCHANGED, its output pointers standing at the round's slot, and beside it what the ban needs.
struct FindBanArgs {
    unsigned long long* ban;     // [count][ban_words] of the chunk: bit p & 63 of word p >> 6 = pool first_pool + row is absent
    int64_t ban_words;           // ceil(pools of the table / 64)
    int32_t* ended;              // [count] of the chunk: 1 once a round found nothing (written by every round's finish)
    int32_t* n_paths;            // [count], at the chunk's first query: written by round 0's finish, incremented by the others
    int32_t round;               // 0 .. max_paths - 1
    int32_t pad;
};
hipError_t launch_find_ban(FindKernel which, const FindArgs& a, const FindBanArgs& b, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// dynamic LDS of a sweep launch: prices (pairs when stage_y), the log-price row, the bin copies, the fee table {γ, 1/γ},
// two doubles per wavefront and the block's two scalars
inline size_t sweep_lds_bytes(int n_pad, int copies, int block, int need_logv, int gtab_n, int stage_y)
{
    const size_t words = (size_t)n_pad * ((stage_y ? 2 : 1) + (need_logv ? 1 : 0) + copies) + 2 * (size_t)gtab_n + 2 * (size_t)(block / 64) + 2;
    return words * sizeof(double);
}
hipError_t prepare_kernels(size_t max_lds_bytes);

// cfmm_quote_rate / cfmm_quote_rate_dev (rate_kernels.h, abi_rate.cpp): cfmm_quote's answer and its marginal rate from one read
// of the pool, one lane per query.  `q` is quote_kernel's view, with two freedoms: q.amount_in null = every amount is 0 (the
// spot-price table), and q.amount_out may be null exactly then.
struct RateArgs {
    QuoteArgs q;
    double* rate;                // [count], never null; NaN for a query that gets NaN in amount_out
};
hipError_t launch_quote_rate(int kind, const RateArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                             hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// cfmm_quote_path_rate / cfmm_quote_path_rate_dev: quote_path_kernel's walk (`p`, exact input) with every hop's rate.
struct PathRateArgs {
    PathArgs p;
    double* rate;                // [count], never null: ((r_0·r_1)·r_2)... over the path's hops
    double* hop_rate;            // [max_hops][count] or null: r_k; NaN in the unused slots
};
hipError_t launch_quote_path_rate(const PathRateArgs& a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

// cfmm_quote_to_rate / cfmm_quote_to_rate_dev (to_rate_kernels.h, abi_limit.cpp): the amount that brings the pool's marginal rate
// down to a limit (to_rate_pool.h) and what it buys, one lane per query.  `q` is quote_kernel's view: q.amount_in carries the
// LIMITS (the value given, as for the exact-output quotes), q.amount_out receives cfmm_quote's answer for the amount and may
// be null.
struct ToRateArgs {
    QuoteArgs q;
    double* amount;              // [count], never null: the amount in; NaN for a bad query
};
hipError_t launch_quote_to_rate(int kind, const ToRateArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// cfmm_swap_limit (swap_limit_kernels.h, abi_swap.cpp): swap_kernel behind a limit on the rate.  `o` is SwapOutArgs with its
// fields re-read: o.max_in carries the RATE limits (never null here; +0.0: no limit for that swap), o.status receives kLimit*.
constexpr int32_t kLimitFilled = 0, kLimitPartial = 1, kLimitNone = 2, kLimitRefused = 3;   // CFMM_LIMIT_* (include/cfmm_amd_limit.h)
struct SwapLimitArgs {
    SwapOutArgs o;
    double* used;                // [count], never null: min(amount_in, the amount to the limit); NaN for a refused swap
};
hipError_t launch_swap_limit(int kind, const SwapLimitArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                             hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

} // namespace cfmm
