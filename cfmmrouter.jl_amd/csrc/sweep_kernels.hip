// sweep_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the per-CFMM arbitrage
// sweep of CFMMRouter.jl and the reductions route! consumes.
//
// What is replaced (paths relative to the reference root):
//   find_arb!(r::Router, v)            src/router.jl:38-42    -> sweep_kernel / sweep_multi (sweep_body)
//   find_arb!(.., ::ProductTwoCoin)    src/cfmms.jl:125-140   -> ProductOps::solve
//   find_arb!(.., ::GeometricMeanTwoCoin) src/cfmms.jl:180-196 -> GeoMeanLogOps::solve (default), GeoMeanOps::solve
//   find_arb!(.., ::UniV3) + helpers   src/cfmms.jl:294-395   -> UniV3Ops::solve_dir
//   GeometricMean / Product, N coins  src/cfmms.jl:57-64 (no find_arb! upstream) -> sweep_ncoin / weighted_pool
//   Curve (StableSwap), N coins       src/cfmms.jl:66-70 (no find_arb! upstream) -> sweep_ncoin / curve_pool, curve_solve
//   acc loop of fn                     src/router.jl:79-83    -> per-lane acc + wave shuffles
//   scatter loop of g! / netflows!     src/router.jl:98-100, :111-119 -> LDS bins + reduce_partials
//                                      (n_tokens > 8192: flow array + gather_chunks / token_fold)
//
// Mapping to the machine.  A two-coin closed form is ~25 dependent flops with no parallelism
// inside a pool, so the unit of work is ONE LANE PER POOL (64 pools per wavefront); the
// data-parallel axis is the pool index, exactly the axis the reference threads over.  Pool
// state is stored as coalesced streams (reserve pairs 16 B + a packed {tokens, fee index} record 8 B per
// lane) and trades leave as one 16 B/lane stream.  Each wavefront owns a private
// copy of the n_tokens netflow bins in LDS and scatters (Lambda - Delta) into it with
// ds_add_f64; the block then folds its copies in a fixed order and writes one partial row to
// global memory.  A second tiny kernel folds the rows, again in a fixed order, so a sweep
// is reproducible bit-for-bit for a fixed launch geometry -- there is no global float atomic.
// The dual scalar is accumulated per lane in tile order and folded with wave shuffles.
//
// Numerics.  Everything is binary64.  This translation unit is compiled with
// -ffp-contract=off and the expressions keep the reference's operation order; with IEEE
// correctly-rounded / and sqrt the ProductTwoCoin and UniV3 trades are bit-identical to the
// reference arithmetic (everything v-independent in the UniV3 forms is prepared at upload with the
// same IEEE operations).  GeometricMeanTwoCoin is evaluated in log space by default (GeoMeanOps
// keeps the reference's pow forms, with the device library's pow).  Against a 60-digit truth both, and the
// N-coin weighted pools, are within a few u·κ·scale (u = 2^-53, κ the conditioning of the exponent; bounds and
// measured ratios in tests/test_gpu_precise.py).  HBM-bound by design: no MFMA (there is no contraction anywhere on this path).
//
// Layout.  This is the only device translation unit (one code object); the device code itself lives in headers, by concern:
//   fast_arith.h      max0, rcp_refined / div_by / fast_sqrt / fast_exp, the window test, pinned()
//   ops_two_coin.h    Trade, Px, the packed-record helpers, ProductOps, GeoMeanOps, GeoMeanLogOps, SolidlyOps
//   ops_univ3.h       UniV3OpsT (UniV3Ops, UniV3OpsLean)
//   sweep_core.h      LDS layout, stage_prices, process_pool, tile loops, finish_row, sweep_kernel, sweep_multi
//   sweep_ncoin.h     weighted_pool, curve_pool (curve_pool.h: the solve), sweep_ncoin
//   fold_kernels.h    reduce_partials, reduce_gather, gather_chunks, token_fold
//   update_kernels.h  update_two_coin, expand_trades, update_ncoin, scatter_records, compact_walks
//   select_kernels.h  select_flag, select_scan, select_emit (cfmm_select_trades)
//   quote_kernels.h   quote_kernel, quote_out_kernel (cfmm_quote, cfmm_quote_out; quote_pool.h: the per-kind forms, src/cfmms.jl:398-449 generalised, and their inverses)
//   quote_path_kernels.h  quote_path_kernel, quote_path_out_kernel (cfmm_quote_path, cfmm_quote_path_out: the same bodies, hop after hop)
//   swap_kernels.h    swap_kernel (cfmm_swap: quote_one's answer, then the pool's new state; swap_pool.h: the per-kind new-state forms)
//   swap_path_kernels.h  swap_path_kernel (cfmm_swap_path: quote_path_kernel's walk, then every hop's new state, all or nothing),
//                        swap_path_out_kernel (cfmm_swap_path_out: quote_path_out_kernel's walk, then the same)
//   swap_out_kernels.h   swap_out_kernel (cfmm_swap_out: quote_out_one's answer, then the pool's new state, with a status per swap)
//   find_path_kernels.h  find_relax and the walk back (cfmm_find_path: the best walk between two tokens, a layer per launch, one lane per pool)
//   size_path_kernels.h  size_path_kernel (cfmm_size_path: the input that maximises a path's gain, one wavefront per path, one lane per trial size)
//   split_paths_kernels.h  split_paths_kernel (cfmm_split_paths: an order's amount spread over its paths, one wavefront per order, one lane per grid point)
//   find_disjoint_kernels.h  find_ban_relax and the walk back (cfmm_find_disjoint_paths: find_path's search with a per-query bitmap of absent pools;
//                            find_out_ban_relax and its walk: cfmm_find_disjoint_paths_out, the same text in the other direction: the header includes its second half once per direction)
//   split_paths_out_kernels.h  split_paths_out_kernel (cfmm_split_paths_out: a wanted amount bought through an order's paths, split_paths_kernel's shape, the hops walked backwards)
//   swap_order_kernels.h  swap_order_kernel, swap_order_out_kernel (cfmm_swap_order, cfmm_swap_order_out: orders executed all or nothing across their paths, eight lanes per order)
//   to_rate_kernels.h, swap_limit_kernels.h   to_rate_kernel, swap_limit_kernel (cfmm_quote_to_rate, cfmm_swap_limit: the amount that brings a pool's marginal rate down to a limit, and the swap that stops there; to_rate_pool.h: the per-kind inverses)
//   rate_kernels.h    rate_kernel, quote_path_rate_kernel (cfmm_quote_rate, cfmm_quote_path_rate: the quote and its marginal rate from one read of the pool; rate_pool.h: the per-kind derivatives)
// What is left here: the kernel table (the one enumeration of the sweep kernels) and the host launchers.

#include "../../include/cfmm_amd.h"
#include "sweep.h"
#include "curve_pool.h"
#include "fast_arith.h"
#include "ops_two_coin.h"
#include "ops_univ3.h"
#include "sweep_core.h"
#include "sweep_ncoin.h"
#include "fold_kernels.h"
#include "update_kernels.h"
#include "select_kernels.h"
#include "quote_kernels.h"
#include "quote_path_kernels.h"
#include "swap_kernels.h"
#include "swap_path_kernels.h"
#include "swap_out_kernels.h"
#include "find_path_kernels.h"   // (and behind it, from its last line, size_path_kernels.h, from that one's split_paths_kernels.h, from that one's find_disjoint_kernels.h, and from that one's split_paths_out_kernels.h, and from that one's swap_order_kernels.h, and from that one's rate_kernels.h, and from that one's swap_limit_kernels.h, which includes to_rate_kernels.h)

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstddef>

namespace cfmm {

hipError_t launch_gather(const int2* chunks, const int* entries, const double* flow, double* chunk_sums, int n_chunks,
                         const int* tok_chunk_off, double* out, int n, const double* acc_rows, int rows, hipStream_t s)
{
    if (n_chunks > 0)
        hipLaunchKernelGGL(gather_chunks, dim3((n_chunks + 15) / 16), dim3(256), 0, s, chunks, entries, flow, chunk_sums,
                           n_chunks);
    hipLaunchKernelGGL(token_fold, dim3((n + 255) / 256 + 1), dim3(256), 0, s, tok_chunk_off, chunk_sums, out, n,
                       acc_rows, rows);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
// Plain launch, or -- when a start/stop event pair is given -- a launch whose events are written by
// the command processor at the kernel's first and last wavefront (hipExtLaunchKernel): that is the
// kernel's own execution span, the quantity rocprofv3 reports, without the ~2.5 us that a
// hipEventRecord / launch / hipEventRecord bracket adds.
static hipError_t launch_k(const void* kernel, dim3 g, dim3 b, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, void** args)
{
    if (e0 && e1) return hipExtLaunchKernel(kernel, g, b, args, lds, s, e0, e1, 0);
    return hipLaunchKernel(kernel, g, b, args, lds, s);
}

// The sweep kernels (82 two-coin instantiations + their 16 lean forms, + 4 N-coin), written down ONCE: this table is what the launchers
// look a kernel up in AND what prepare_kernels walks, so a kernel that can be launched cannot miss its LDS attribute.
// Which (family, arithmetic) pairs exist is the constructor below: per family {full-range, fast, auto} x {materialising,
// fused} x {512, 1024 threads}; the reference-order GeometricMean forms, Solidly and the N-coin families run full-range
// only (the N-coin ones at 512 threads), and so does the large-market mode (GBINS) of every family, at 512 threads.
// The last dimension is the lean form (sweep_core.h sweep_body<..., LEAN>; chosen by launch_plan.h lean_launch): the fused
// launch at 512 threads and ProductTwoCoin, log-space GeometricMean and UniV3 (with heads) at 1024, fast and auto arithmetic.
enum KernelFamily { kFamProduct, kFamGeoMean, kFamGeoMeanLog, kFamSolidly, kFamUniV3, kFamUniV3Lean, kFamMulti, kFamWeighted, kFamCurve, kFamilies };
struct SweepKernelTable {
    static constexpr int kGbinsSlot = 3;   // large-market mode sits behind the three arithmetics
    // [family][arithmetic, or kGbinsSlot][block == kBigBlock][materialising][lean]; null: no such kernel
    const void* fn[kFamilies][4][2][2][2] = {};

    template <class K> static const void* ptr(K* kernel) { return reinterpret_cast<const void*>(kernel); }
    template <class Ops, int ARITH> void sweep(int f)
    {
        fn[f][ARITH][0][1][0] = ptr(&sweep_kernel<Ops, true, kMidBlock, false, ARITH>);
        fn[f][ARITH][0][0][0] = ptr(&sweep_kernel<Ops, false, kMidBlock, false, ARITH>);
        fn[f][ARITH][1][1][0] = ptr(&sweep_kernel<Ops, true, kBigBlock, false, ARITH>);
        fn[f][ARITH][1][0][0] = ptr(&sweep_kernel<Ops, false, kBigBlock, false, ARITH>);
    }
    template <class Ops, int ARITH> void sweep_lean(int f)
    {
        fn[f][ARITH][1][1][1] = ptr(&sweep_kernel<Ops, true, kBigBlock, false, ARITH, true>);
        fn[f][ARITH][1][0][1] = ptr(&sweep_kernel<Ops, false, kBigBlock, false, ARITH, true>);
    }
    template <int ARITH> void lean()
    {
        fn[kFamMulti][ARITH][0][1][1] = ptr(&sweep_multi<true, kMidBlock, false, ARITH, true>);
        fn[kFamMulti][ARITH][0][0][1] = ptr(&sweep_multi<false, kMidBlock, false, ARITH, true>);
        sweep_lean<ProductOps, ARITH>(kFamProduct);
        sweep_lean<GeoMeanLogOps, ARITH>(kFamGeoMeanLog);
        sweep_lean<UniV3Ops, ARITH>(kFamUniV3);
    }
    template <class Ops> void sweep_all(int f) { sweep<Ops, kArithFull>(f); sweep<Ops, kArithFast>(f); sweep<Ops, kArithAuto>(f); }
    template <class Ops> void sweep_gbins(int f)
    {
        fn[f][kGbinsSlot][0][1][0] = ptr(&sweep_kernel<Ops, true, kMidBlock, true, kArithFull>);
        fn[f][kGbinsSlot][0][0][0] = ptr(&sweep_kernel<Ops, false, kMidBlock, true, kArithFull>);
    }
    template <int ARITH> void multi()
    {
        fn[kFamMulti][ARITH][1][1][0] = ptr(&sweep_multi<true, kBigBlock, false, ARITH>);
        fn[kFamMulti][ARITH][1][0][0] = ptr(&sweep_multi<false, kBigBlock, false, ARITH>);
        fn[kFamMulti][ARITH][0][1][0] = ptr(&sweep_multi<true, kMidBlock, false, ARITH>);
        fn[kFamMulti][ARITH][0][0][0] = ptr(&sweep_multi<false, kMidBlock, false, ARITH>);
    }
    template <class F> void ncoin(int f)
    {
        fn[f][kArithFull][0][1][0] = ptr(&sweep_ncoin<F, true>);
        fn[f][kArithFull][0][0][0] = ptr(&sweep_ncoin<F, false>);
    }
    SweepKernelTable()
    {
        fn[kFamMulti][kGbinsSlot][0][1][0] = ptr(&sweep_multi<true, kMidBlock, true, kArithFull>);
        fn[kFamMulti][kGbinsSlot][0][0][0] = ptr(&sweep_multi<false, kMidBlock, true, kArithFull>);
        multi<kArithFull>(); multi<kArithFast>(); multi<kArithAuto>();
        lean<kArithFast>(); lean<kArithAuto>();
        ncoin<WeightedFamily>(kFamWeighted);
        ncoin<CurveFamily>(kFamCurve);
        sweep_all<ProductOps>(kFamProduct);
        sweep<GeoMeanOps, kArithFull>(kFamGeoMean);
        sweep<SolidlyOps, kArithFull>(kFamSolidly);
        sweep_all<GeoMeanLogOps>(kFamGeoMeanLog);
        sweep_all<UniV3Ops>(kFamUniV3);
        sweep_all<UniV3OpsLean>(kFamUniV3Lean);
        sweep_gbins<ProductOps>(kFamProduct);
        sweep_gbins<GeoMeanOps>(kFamGeoMean);
        sweep_gbins<GeoMeanLogOps>(kFamGeoMeanLog);
        sweep_gbins<SolidlyOps>(kFamSolidly);
        sweep_gbins<UniV3Ops>(kFamUniV3);   // (never requested: launch_sweep sends large markets to the lean walk)
        sweep_gbins<UniV3OpsLean>(kFamUniV3Lean);
    }
    // null: no such kernel -- there is no falling through to another one
    const void* find(int f, bool mat, int block, bool gbins, int arith, bool lean) const
    {
        if ((block != kMidBlock && block != kBigBlock) || arith < kArithFull || arith > kArithAuto || (gbins && (arith != kArithFull || lean)))
            return nullptr;
        return fn[f][gbins ? kGbinsSlot : arith][block == kBigBlock][mat][lean];
    }
};
static const SweepKernelTable kSweepKernels;

// every kernel of the table may use the whole LDS of a CU
hipError_t prepare_kernels(size_t max_lds_bytes)
{
    const void* const* kernels = &kSweepKernels.fn[0][0][0][0][0];
    for (size_t k = 0; k < sizeof(SweepKernelTable::fn) / sizeof(void*); ++k) {
        if (!kernels[k]) continue;
        hipError_t e = hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// every sweep launch: the kernel comes from the table or the launch fails
static hipError_t launch_family(int family, bool gbins, const LaunchCfg& c, bool mat, hipStream_t s, void** args)
{
    const void* kernel = kSweepKernels.find(family, mat, c.block, gbins, c.arith, c.lean);
    if (!kernel) return hipErrorInvalidDeviceFunction;
    return launch_k(kernel, dim3(c.grid), dim3(c.block), c.lds_bytes, s, c.ev_start, c.ev_stop, args);
}

// the kernels' parameters: SweepLaunch's four leading scalars, then its tail
struct SweepParams {
    SweepLaunch la;
    void* args[kSweepScalars + 1];
    explicit SweepParams(const SweepLaunch& l) : la(l), args{&la.desc, &la.v, &la.reverse, &la.n, &la.tail} {}
};

hipError_t launch_multi(bool gbins, const SweepLaunch& la, const LaunchCfg& c, bool mat, hipStream_t s)
{
    SweepParams p(la);
    return launch_family(kFamMulti, gbins, c, mat, s, p.args);
}

hipError_t launch_sweep(int kind, bool reference_order, bool heads, bool gbins, const SweepLaunch& la, const LaunchCfg& c, bool mat,
                        hipStream_t s)
{
    int family;
    switch (kind) {
    case CFMM_KIND_PRODUCT: family = kFamProduct; break;
    case CFMM_KIND_GEOMEAN: family = reference_order ? kFamGeoMean : kFamGeoMeanLog; break;
    case CFMM_KIND_UNIV3: family = heads && !gbins ? kFamUniV3 : kFamUniV3Lean; break;
    case CFMM_KIND_SOLIDLY: family = kFamSolidly; break;
    default: return hipErrorInvalidDeviceFunction;
    }
    SweepParams p(la);
    return launch_family(family, gbins, c, mat, s, p.args);
}

hipError_t launch_ncoin(int kind, const NCoinPools& pools, const SweepArgs& a, bool gbins, const LaunchCfg& c, bool mat, hipStream_t s)
{
    if (a.m <= 0) return hipSuccess;
    if (kind != CFMM_KIND_WEIGHTED && kind != CFMM_KIND_CURVE) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<NCoinPools*>(&pools), const_cast<SweepArgs*>(&a)};
    return launch_family(kind == CFMM_KIND_WEIGHTED ? kFamWeighted : kFamCurve, gbins, c, mat, s, args);
}

hipError_t launch_reduce(const double* partials, int rows, int n1, int pitch, double* out, hipStream_t s, hipEvent_t e0, hipEvent_t e1,
                         HostOut host, ArmWord arm)
{
    dim3 g(fold_grid(n1));
    void* args[] = {&partials, &rows, &n1, &pitch, &out, &host, &arm};
    return launch_k(reinterpret_cast<const void*>(&reduce_partials<kFoldBlock>), g, dim3(kFoldBlock), 0, s, e0, e1, args);
}

hipError_t launch_update_two_coin(double2* R, const double* gamma, const double2* Delta, const double2* Lambda,
                                  const double2* Over, int compact, double2* Q, const double* eta, int64_t m, int* left_window,
                                  hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_two_coin, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, R, gamma, Delta, Lambda, Over,
                       compact, Q, eta, (long long)m, left_window);
    return hipGetLastError();
}

hipError_t launch_update_ncoin(int kind, double* R, double* q, const double* par, const double2* glg, const double* Delta,
                               const double* Lambda, int n_coins, int64_t m, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    const dim3 g((unsigned)((m + 255) / 256)), b(256);
    if (kind == CFMM_KIND_CURVE)
        hipLaunchKernelGGL(update_ncoin<CurveFamily>, g, b, 0, s, R, q, par, glg, Delta, Lambda, n_coins, (long long)m);
    else
        hipLaunchKernelGGL(update_ncoin<WeightedFamily>, g, b, 0, s, R, q, par, glg, Delta, Lambda, n_coins, (long long)m);
    return hipGetLastError();
}

hipError_t launch_expand_trades(const double2* rec, const double2* ovA, const double2* ovB, double2* Delta, double2* Lambda,
                                int64_t m, hipStream_t s)
{
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(expand_trades, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, rec, ovA, ovB, Delta, Lambda,
                       (long long)m);
    return hipGetLastError();
}

hipError_t launch_scatter_records(const ScatterArgs& a, hipStream_t s)
{
    if (a.total <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_records, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_compact_walks(const int4* old_walk, const int4* new_walk, int4* walk_out, const TickRec* old_ticks, TickRec* ticks,
                                double* thr, int64_t m, int64_t tail, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (m <= 0) return hipErrorInvalidValue;
    static_assert(sizeof(TickRec) == 64 && offsetof(TickRec, thr) == 40, "compact_walks: piece 2 of a record is {rout, thr}");
    long long mm = m, tt = tail;
    void* args[] = {&old_walk, &new_walk, &walk_out, &old_ticks, &ticks, &thr, &mm, &tt};
    const long long blocks = (mm * kCompactGroup + 255) / 256;
    return launch_k(reinterpret_cast<const void*>(&compact_walks), dim3((unsigned)blocks), dim3(256), 0, s, e0, e1, args);
}

hipError_t launch_select_count(const SelectArgs& a, bool ragged, long long* total_host, hipStream_t s, hipEvent_t* ev)
{
    if (a.m <= 0) return hipErrorInvalidValue;
    long long blocks = select_blocks(a.m);
    const int* counts = a.counts;
    long long* base = a.base;
    void* flag_args[] = {const_cast<SelectArgs*>(&a)};
    const void* flag = ragged ? reinterpret_cast<const void*>(&select_flag<true>) : reinterpret_cast<const void*>(&select_flag<false>);
    hipError_t e = launch_k(flag, dim3((unsigned)blocks), dim3(kSelBlock), 0, s, ev ? ev[0] : nullptr, ev ? ev[1] : nullptr, flag_args);
    if (e != hipSuccess) return e;
    void* scan_args[] = {&counts, &base, &blocks, &total_host};
    return launch_k(reinterpret_cast<const void*>(&select_scan), dim3(1), dim3(kSelScanChunk), 0, s, ev ? ev[2] : nullptr,
                    ev ? ev[3] : nullptr, scan_args);
}

hipError_t launch_select_emit(const SelectArgs& a, bool ragged, hipStream_t s, hipEvent_t* ev)
{
    if (a.m <= 0) return hipErrorInvalidValue;
    void* args[] = {const_cast<SelectArgs*>(&a)};
    const void* emit = ragged ? reinterpret_cast<const void*>(&select_emit<true>) : reinterpret_cast<const void*>(&select_emit<false>);
    return launch_k(emit, dim3((unsigned)select_blocks(a.m)), dim3(kSelBlock), 0, s, ev ? ev[4] : nullptr, ev ? ev[5] : nullptr, args);
}

hipError_t launch_reduce_gather(const double* partials, int rows, int n1, int pitch, double* out, hipStream_t s, const PeerSet& ps,
                                hipEvent_t e0, hipEvent_t e1)
{
    dim3 g(fold_grid(n1));
    void* args[] = {&partials, &rows, &n1, &pitch, &out, const_cast<PeerSet*>(&ps)};
    return launch_k(reinterpret_cast<const void*>(&reduce_gather<kFoldBlock>), g, dim3(kFoldBlock), 0, s, e0, e1, args);
}

// one lane per query, at most one machine of resident threads (the lanes stride over the rest)
static hipError_t launch_quote_grid(const void* kernel, int64_t count, void** args, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    const int64_t blocks = std::min<int64_t>((count + kQuoteBlock - 1) / kQuoteBlock, kResidentThreads / kQuoteBlock);
    return launch_k(kernel, dim3((unsigned)blocks), dim3(kQuoteBlock), 0, s, e0, e1, args);
}

static hipError_t launch_quote_k(const void* kernel, const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s,
                                 hipEvent_t e0, hipEvent_t e1)
{
    void* args[] = {const_cast<QuoteArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.count, args, s, e0, e1);
}

hipError_t launch_quote(int kind, const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.count <= 0 || a.m <= 0) return hipErrorInvalidValue;
    const void* kernel = nullptr;   // no such kernel: there is no falling through to another one
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&quote_kernel<decltype(K)::value>); }, [] {});
    if (!kernel) return hipErrorInvalidDeviceFunction;
    return launch_quote_k(kernel, a, u, n, s, e0, e1);
}

hipError_t launch_quote_out(int kind, const QuoteArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0,
                            hipEvent_t e1)
{
    if (a.count <= 0 || a.m <= 0) return hipErrorInvalidValue;
    const void* kernel = nullptr;   // no such kernel: there is no falling through to another one
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&quote_out_kernel<decltype(K)::value>); }, [] {});
    if (!kernel) return hipErrorInvalidDeviceFunction;
    return launch_quote_k(kernel, a, u, n, s, e0, e1);
}

// one lane per path, the same grid rule
hipError_t launch_quote_path(bool exact_out, const PathArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.count <= 0 || a.nseg <= 0 || a.max_hops < 1 || a.max_hops > CFMM_MAX_PATH_HOPS) return hipErrorInvalidValue;
    void* args[] = {const_cast<PathArgs*>(&a)};
    const void* kernel = exact_out ? reinterpret_cast<const void*>(&quote_path_out_kernel<kQuoteBlock>) : reinterpret_cast<const void*>(&quote_path_kernel<kQuoteBlock>);
    return launch_quote_grid(kernel, a.count, args, s, e0, e1);
}

// cfmm_quote_rate / cfmm_quote_path_rate: launch_quote's and launch_quote_path's rules and grids.  The kernels are NAMED at the
// end of this file (rate_kernel_of, path_rate_kernel), behind every other launcher: templates are emitted in the order they are
// named, so every kernel the translation unit had before keeps its function number, labels and bytes.
static const void* rate_kernel_of(int kind);
static const void* path_rate_kernel();

hipError_t launch_quote_rate(int kind, const RateArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.q.count <= 0 || a.q.m <= 0 || !a.rate || (!a.q.amount_out && a.q.amount_in)) return hipErrorInvalidValue;
    const void* kernel = rate_kernel_of(kind);   // no such kernel: there is no falling through to another one
    if (!kernel) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<RateArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.q.count, args, s, e0, e1);
}

hipError_t launch_quote_path_rate(const PathRateArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.p.count <= 0 || a.p.nseg <= 0 || a.p.max_hops < 1 || a.p.max_hops > CFMM_MAX_PATH_HOPS || !a.p.answer || !a.rate) return hipErrorInvalidValue;
    void* args[] = {const_cast<PathRateArgs*>(&a)};
    return launch_quote_grid(path_rate_kernel(), a.p.count, args, s, e0, e1);
}

// cfmm_quote_to_rate and cfmm_swap_limit: launch_quote_rate's and launch_swap's rules and grids.  Their kernels are named at the
// end of this file too (to_rate_kernel_of, swap_limit_kernel_of), behind the rate kernels, for the same reason.
static const void* to_rate_kernel_of(int kind);
static const void* swap_limit_kernel_of(int kind);

hipError_t launch_quote_to_rate(int kind, const ToRateArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.q.count <= 0 || a.q.m <= 0 || !a.amount || !a.q.amount_in) return hipErrorInvalidValue;
    const void* kernel = to_rate_kernel_of(kind);   // no such kernel: there is no falling through to another one
    if (!kernel) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<ToRateArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.q.count, args, s, e0, e1);
}

hipError_t launch_swap_limit(int kind, const SwapLimitArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.o.s.q.count <= 0 || a.o.s.q.m <= 0 || !a.o.max_in || !a.o.status || !a.used) return hipErrorInvalidValue;
    const void* kernel = swap_limit_kernel_of(kind);   // no such kernel: there is no falling through to another one
    if (!kernel) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<SwapLimitArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.o.s.q.count, args, s, e0, e1);
}

// one lane per swap of the wave, the same grid rule
hipError_t launch_swap(int kind, const SwapArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.q.count <= 0 || a.q.m <= 0) return hipErrorInvalidValue;
    const void* kernel = nullptr;   // no such kernel: there is no falling through to another one
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&swap_kernel<decltype(K)::value>); }, [] {});
    if (!kernel) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<SwapArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.q.count, args, s, e0, e1);
}

// one lane per path of the wave, the same grid rule
hipError_t launch_swap_path(const SwapPathArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.count <= 0 || a.stride < a.count || a.nseg <= 0 || a.max_hops < 1 || a.max_hops > CFMM_MAX_PATH_HOPS || !a.hops || !a.price || !a.status)
        return hipErrorInvalidValue;
    void* args[] = {const_cast<SwapPathArgs*>(&a)};
    return launch_quote_grid(reinterpret_cast<const void*>(&swap_path_kernel<kQuoteBlock>), a.count, args, s, e0, e1);
}

// cfmm_swap_out: one lane per swap of the wave, the same grid rule
hipError_t launch_swap_out(int kind, const SwapOutArgs& a, const UniV3Pools& u, const NCoinPools& n, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.s.q.count <= 0 || a.s.q.m <= 0 || !a.status) return hipErrorInvalidValue;
    const void* kernel = nullptr;   // no such kernel: there is no falling through to another one
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&swap_out_kernel<decltype(K)::value>); }, [] {});
    if (!kernel) return hipErrorInvalidDeviceFunction;
    void* args[] = {const_cast<SwapOutArgs*>(&a), const_cast<UniV3Pools*>(&u), const_cast<NCoinPools*>(&n)};
    return launch_quote_grid(kernel, a.s.q.count, args, s, e0, e1);
}

// cfmm_swap_path_out: launch_swap_path's rule
hipError_t launch_swap_path_out(const SwapPathArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.count <= 0 || a.stride < a.count || a.nseg <= 0 || a.max_hops < 1 || a.max_hops > CFMM_MAX_PATH_HOPS || !a.hops || !a.price || !a.status)
        return hipErrorInvalidValue;
    void* args[] = {const_cast<SwapPathArgs*>(&a)};
    return launch_quote_grid(reinterpret_cast<const void*>(&swap_path_out_kernel<kQuoteBlock>), a.count, args, s, e0, e1);
}

// cfmm_find_path: the per-query kernels take launch_quote_grid's rule without the stride (one lane per query of the chunk);
// the per-pool kernels one block per tile of the table and one grid row per kFindLaneQueries queries
// (the grid and LDS of a launch of `role`, an exact-input FindKernel: launch_find and launch_find_ban)
static hipError_t find_launch_shape(int role, const FindArgs& a, dim3& grid, size_t& lds_bytes)
{
    if (a.count <= 0 || a.stride < a.count || a.nseg <= 0 || a.n_tokens <= 0 || a.max_hops < 1 || a.max_hops > CFMM_MAX_PATH_HOPS)
        return hipErrorInvalidValue;
    const int64_t qblocks = (a.count + kFindBlock - 1) / kFindBlock, qrows = (a.count + kFindLaneQueries - 1) / kFindLaneQueries;
    const bool per_pool = role == kFindRelax || role == kFindClaim;
    if (role != kFindInit && role != kFindSelect && role != kFindFinish && (a.layer < 1 || a.layer > a.max_hops)) return hipErrorInvalidValue;
    if (per_pool && (a.tiles <= 0 || a.tiles > 0x7fffffffll || qrows > 65535)) return hipErrorInvalidValue;
    if (qblocks > 0x7fffffffll) return hipErrorInvalidValue;
    const bool lds = role == kFindRelax && a.group > 0;
    if (lds && (a.group > kFindLaneQueries || a.group > find_lds_group(a.n_tokens) || a.tiles_per_block < 1)) return hipErrorInvalidValue;
    grid = per_pool ? dim3((unsigned)a.tiles, (unsigned)qrows) : dim3((unsigned)qblocks);
    lds_bytes = 0;
    if (lds) {
        const int64_t rows = (a.count + a.group - 1) / a.group;
        if (rows > 65535) return hipErrorInvalidValue;
        grid = dim3((unsigned)((a.tiles + a.tiles_per_block - 1) / a.tiles_per_block), (unsigned)rows);
        lds_bytes = (size_t)a.group * (size_t)a.n_tokens * sizeof(unsigned long long);
    }
    return hipSuccess;
}

hipError_t launch_find(FindKernel which, const FindArgs& a, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    dim3 grid;
    size_t lds_bytes;
    const hipError_t shape = find_launch_shape(which >= kFindOutFirst ? which - kFindOutFirst : which, a, grid, lds_bytes);   // (cfmm_find_path_out's kernels take the same grids)
    if (shape != hipSuccess) return shape;
    const bool lds = lds_bytes > 0;
    const void* kernel;
    switch (which) {
    case kFindInit: kernel = reinterpret_cast<const void*>(&find_init<kFindBlock>); break;
    case kFindRelax: kernel = lds ? reinterpret_cast<const void*>(&find_relax<kFindBlock, true>) : reinterpret_cast<const void*>(&find_relax<kFindBlock, false>); break;
    case kFindSelect: kernel = reinterpret_cast<const void*>(&find_select<kFindBlock>); break;
    case kFindClaim: kernel = reinterpret_cast<const void*>(&find_claim<kFindBlock>); break;
    case kFindAdvance: kernel = reinterpret_cast<const void*>(&find_advance<kFindBlock>); break;
    case kFindFinish: kernel = reinterpret_cast<const void*>(&find_finish<kFindBlock>); break;
    case kFindOutInit: kernel = reinterpret_cast<const void*>(&find_out_init<kFindBlock>); break;
    case kFindOutRelax: kernel = lds ? reinterpret_cast<const void*>(&find_out_relax<kFindBlock, true>) : reinterpret_cast<const void*>(&find_out_relax<kFindBlock, false>); break;
    case kFindOutSelect: kernel = reinterpret_cast<const void*>(&find_out_select<kFindBlock>); break;
    case kFindOutClaim: kernel = reinterpret_cast<const void*>(&find_out_claim<kFindBlock>); break;
    case kFindOutAdvance: kernel = reinterpret_cast<const void*>(&find_out_advance<kFindBlock>); break;
    case kFindOutFinish: kernel = reinterpret_cast<const void*>(&find_out_finish<kFindBlock>); break;
    default: return hipErrorInvalidDeviceFunction;   // no such kernel
    }
    void* args[] = {const_cast<FindArgs*>(&a)};
    return launch_k(kernel, grid, dim3(kFindBlock), lds_bytes, s, e0, e1, args);
}

// cfmm_size_path: one wavefront per path, kSizeBlock / 64 paths per block, at most max_blocks blocks.  (Behind every other
// launcher: the kernel is instantiated last, so every kernel before it keeps its function number and labels.)
hipError_t launch_size_path(const SizeArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.p.count <= 0 || a.p.nseg <= 0 || a.p.max_hops < 1 || a.p.max_hops > CFMM_MAX_PATH_HOPS || a.rounds < 1 ||
        a.rounds > CFMM_MAX_SIZE_ROUNDS || max_blocks < 1 || !a.p.answer || !a.amount_out || !a.gain || !a.status)
        return hipErrorInvalidValue;
    constexpr int64_t per_block = kSizeBlock / CFMM_SIZE_POINTS;
    const int64_t blocks = std::min<int64_t>({(a.p.count + per_block - 1) / per_block, max_blocks, (int64_t)0x7fffffff});
    void* args[] = {const_cast<SizeArgs*>(&a)};
    return launch_k(reinterpret_cast<const void*>(&size_path_kernel<kSizeBlock>), dim3((unsigned)blocks), dim3(kSizeBlock), 0, s, e0, e1, args);
}

// cfmm_split_paths: one wavefront per order, kSplitBlock / 64 orders per block, at most max_blocks blocks.  (Behind every other
// launcher, for launch_size_path's reason.)
hipError_t launch_split_paths(const SplitArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.orders <= 0 || a.p.count <= 0 || a.p.nseg <= 0 || a.p.max_hops < 1 || a.p.max_hops > CFMM_MAX_PATH_HOPS || a.rounds < 1 ||
        a.rounds > CFMM_MAX_SPLIT_ROUNDS || max_blocks < 1 || !a.order_first || !a.amount || !a.p.answer || !a.path_out || !a.total || !a.status)
        return hipErrorInvalidValue;
    constexpr int64_t per_block = kSplitBlock / CFMM_SPLIT_POINTS;
    const int64_t blocks = std::min<int64_t>({(a.orders + per_block - 1) / per_block, max_blocks, (int64_t)0x7fffffff});
    void* args[] = {const_cast<SplitArgs*>(&a)};
    return launch_k(reinterpret_cast<const void*>(&split_paths_kernel<kSplitBlock>), dim3((unsigned)blocks), dim3(kSplitBlock), 0, s, e0, e1, args);
}

// cfmm_find_disjoint_paths / cfmm_find_disjoint_paths_out: launch_find's grids for the four kernels per direction that know the ban.  (Behind every other launcher, for
// launch_size_path's reason.)
hipError_t launch_find_ban(FindKernel which, const FindArgs& a, const FindBanArgs& b, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    dim3 grid;
    size_t lds_bytes;
    const hipError_t shape = find_launch_shape(which >= kFindOutFirst ? which - kFindOutFirst : which, a, grid, lds_bytes);   // (the backwards kernels take the same grids)
    if (shape != hipSuccess) return shape;
    if (!b.ban || b.ban_words < 1 || !b.ended || !b.n_paths || b.round < 0 || b.round >= CFMM_MAX_SPLIT_PATHS) return hipErrorInvalidValue;
    const void* kernel;
    switch (which) {
    case kFindInit: kernel = reinterpret_cast<const void*>(&find_ban_init<kFindBlock>); break;
    case kFindRelax: kernel = lds_bytes > 0 ? reinterpret_cast<const void*>(&find_ban_relax<kFindBlock, true>) : reinterpret_cast<const void*>(&find_ban_relax<kFindBlock, false>); break;
    case kFindClaim: kernel = reinterpret_cast<const void*>(&find_ban_claim<kFindBlock>); break;
    case kFindFinish: kernel = reinterpret_cast<const void*>(&find_ban_finish<kFindBlock>); break;
    // cfmm_find_disjoint_paths_out (behind the four above: templates are emitted in the order they are named)
    case kFindOutInit: kernel = reinterpret_cast<const void*>(&find_out_ban_init<kFindBlock>); break;
    case kFindOutRelax: kernel = lds_bytes > 0 ? reinterpret_cast<const void*>(&find_out_ban_relax<kFindBlock, true>) : reinterpret_cast<const void*>(&find_out_ban_relax<kFindBlock, false>); break;
    case kFindOutClaim: kernel = reinterpret_cast<const void*>(&find_out_ban_claim<kFindBlock>); break;
    case kFindOutFinish: kernel = reinterpret_cast<const void*>(&find_out_ban_finish<kFindBlock>); break;
    default: return hipErrorInvalidDeviceFunction;   // select and advance know no ban: launch_find
    }
    void* args[] = {const_cast<FindArgs*>(&a), const_cast<FindBanArgs*>(&b)};
    return launch_k(kernel, grid, dim3(kFindBlock), lds_bytes, s, e0, e1, args);
}

// cfmm_split_paths_out: launch_split_paths' checks and grid.  (Behind every other launcher, for launch_size_path's reason.)
hipError_t launch_split_paths_out(const SplitArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.orders <= 0 || a.p.count <= 0 || a.p.nseg <= 0 || a.p.max_hops < 1 || a.p.max_hops > CFMM_MAX_PATH_HOPS || a.rounds < 1 ||
        a.rounds > CFMM_MAX_SPLIT_ROUNDS || max_blocks < 1 || !a.order_first || !a.amount || !a.p.answer || !a.path_out || !a.total || !a.status)
        return hipErrorInvalidValue;
    constexpr int64_t per_block = kSplitBlock / CFMM_SPLIT_POINTS;
    const int64_t blocks = std::min<int64_t>({(a.orders + per_block - 1) / per_block, max_blocks, (int64_t)0x7fffffff});
    void* args[] = {const_cast<SplitArgs*>(&a)};
    return launch_k(reinterpret_cast<const void*>(&split_paths_out_kernel<kSplitBlock>), dim3((unsigned)blocks), dim3(kSplitBlock), 0, s, e0, e1, args);
}

// cfmm_swap_order / cfmm_swap_order_out: eight lanes per order of the wave, kOrderBlock / 8 orders per block, at most max_blocks
// blocks.  (Behind every other launcher, for launch_size_path's reason.)
hipError_t launch_swap_order(bool exact_out, const SwapOrderArgs& a, int64_t max_blocks, hipStream_t s, hipEvent_t e0, hipEvent_t e1)
{
    if (a.orders <= 0 || a.p.count <= 0 || a.p.stride != a.p.count || a.p.nseg <= 0 || a.p.max_hops < 1 || a.p.max_hops > CFMM_MAX_PATH_HOPS ||
        max_blocks < 1 || !a.order_first || !a.p.amount_out || !a.p.hops || !a.p.price || !a.p.status || !a.total || !a.status)
        return hipErrorInvalidValue;
    constexpr int64_t per_block = kOrderBlock / kOrderLanes;
    const int64_t blocks = std::min<int64_t>({(a.orders + per_block - 1) / per_block, max_blocks, (int64_t)0x7fffffff});
    void* args[] = {const_cast<SwapOrderArgs*>(&a)};
    const void* kernel = exact_out ? reinterpret_cast<const void*>(&swap_order_out_kernel<kOrderBlock>) : reinterpret_cast<const void*>(&swap_order_kernel<kOrderBlock>);
    return launch_k(kernel, dim3((unsigned)blocks), dim3(kOrderBlock), 0, s, e0, e1, args);
}

// The kernels of launch_quote_rate and launch_quote_path_rate, named here and nowhere else.  (Behind every launcher, for
// launch_size_path's reason.)
static const void* rate_kernel_of(int kind)
{
    const void* kernel = nullptr;
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&rate_kernel<decltype(K)::value>); }, [] {});
    return kernel;
}
static const void* path_rate_kernel() { return reinterpret_cast<const void*>(&quote_path_rate_kernel<kQuoteBlock>); }

// The kernels of launch_quote_to_rate and launch_swap_limit, named here and nowhere else, behind the rate kernels.
static const void* to_rate_kernel_of(int kind)
{
    const void* kernel = nullptr;
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&to_rate_kernel<decltype(K)::value>); }, [] {});
    return kernel;
}
static const void* swap_limit_kernel_of(int kind)
{
    const void* kernel = nullptr;
    with_kind(kind, [&](auto K) { kernel = reinterpret_cast<const void*>(&swap_limit_kernel<decltype(K)::value>); }, [] {});
    return kernel;
}

} // namespace cfmm
