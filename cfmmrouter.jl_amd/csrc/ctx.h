// ctx.h -- internal: the context behind the C ABI (include/cfmm_amd.h) and what the abi_*.cpp translation units
// share.  Host-side only.  There is no CPU fallback anywhere behind this header: without a gfx950 device every
// entry point that needs one fails with CFMM_ERR_HIP.
//
//   devbuf.h          DevBuf<T>: the one owner of a device array (every Segment / context array below is one)
//   hostres.h         PinnedBuf<T>, Event, Stream: the owners of pinned memory, events and streams; TradeStaging
//   granule.h         the self-validating output granule {tag, 32 bits}, for host and device code
//   abi_context.cpp   create / destroy / options / streams / introspection, the raw create / destroy calls of every owner
//   abi_upload.cpp    pool validation + upload (src/cfmms.jl:76-111, :152-165, :226-245), prepared constants
//   launch_plan.cpp   the launch geometry of one evaluation, as a pure function (launch_plan.h: no HIP, no context)
//   abi_sweep.cpp     applies the plan (fee tables, buffers), one evaluation = sweep launches + row fold
//   abi_handover.cpp  how an evaluation's result crosses to the host: host-pointer sweeps, the granule wait, pre-armed evaluations
//   abi_trades.cpp    trade download / device views, the selection of the trades worth executing, update_reserves!,
//                     reserves / prices read-back
//   abi_update.cpp    sparse pool-state updates (cfmm_pools_set_reserves / _set_curve / _set_prices / _set_ticks)
//   ladder_store.h    LadderStore: a UniV3 segment's tick ladders on the host, one pool's replaceable (no HIP)
//   abi_quote.cpp     exact-input swap quotes (cfmm_quote / cfmm_quote_dev; forward_trade generalised) and their inverses, the
//                     exact-output quotes (cfmm_quote_out / cfmm_quote_out_dev)
//   abi_quote_path.cpp  multi-hop path quotes across segments (cfmm_quote_path / _out and their _dev forms; path_checks.h: the
//                     HIP-free checks)
//   abi_swap.cpp      exact-input swaps that move the pools, and by a direction their exact-output form cfmm_swap_out
//                     (cfmm_swap: the quote, then R + γΔ − Λ; swap_waves.h: the HIP-free wave numbering of repeated rows)
//   abi_swap_path.cpp swap PATHS that move their pools, all or nothing, in both directions (cfmm_swap_path,
//                     cfmm_swap_path_out; swap_path_checks.h: the HIP-free checks beyond path_checks.h), and swap_paths_run, the
//                     driver of every executing path entry (swap_path_waves.h: the HIP-free wave planner and its
//                     pool table; swap_fill.h: the HIP-free fill in launch order, its inverse and the UniV3 landing rule)
//   abi_swap_order.cpp ORDERS executed all or nothing across their 1 .. 8 paths, in both directions (cfmm_swap_order,
//                     cfmm_swap_order_out: the checks, order_checks.h, HIP-free; the call is swap_paths_run)
//   abi_find_path.cpp the best swap walk between two tokens, found on the device (cfmm_find_path; find_checks.h: the HIP-free
//                     checks and the chunking rule)
//   abi_size_path.cpp the input of a path that maximises its gain (cfmm_size_path; size_checks.h: the HIP-free checks, size_grid.h:
//                     the search's arithmetic, shared with the kernel)
//   abi_split_paths.cpp an order's amount spread over several paths (cfmm_split_paths; split_checks.h: the HIP-free checks,
//                     split_grid.h: the search's arithmetic, shared with the kernel)
//                     and bought through several paths (cfmm_split_paths_out: the same file, checks and scratch;
//                     split_out_grid.h: what its search has of its own)
//   path_rig.h        the rig of the read-only path entries (PathRig below: quote_path, size_path, split_paths)
//   split_search.h    the search a multi-device parent runs on the host for the last two (no HIP)
//   seg_view.h        what those eight share, on top of this header: a segment as their kernels and their checks see it
//   stage_layout.h    ... and how each carves its pinned staging buffer into columns (no HIP)
//   shard_split.h     shard_range, and a parent's queries bucketed by shard (no HIP)
//   abi_route.cpp     route! in one call (L-BFGS-B + objectives), the bare solver
//   abi_multi.cpp     single-process multi-device parents
//   abi_peers.cpp     one process per GPU: peer buffers, cfmm_set_peers
//   abi_rccl.cpp      one process per GPU: the all-reduce through RCCL (cfmm_set_rccl_comm, cfmm_rccl_init_rank)
#pragma once

#include "../../include/cfmm_amd.h"
#include "../../include/cfmm_amd_split.h"
#include "../../include/cfmm_amd_split_out.h"
#include "devbuf.h"
#include "hostres.h"
#include "ladder_store.h"
#include "launch_plan.h"
#include "shard_split.h"
#include "swap_fill.h"
#include "sweep.h"

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace cfmm {

// Every resource has one owner (devbuf.h, hostres.h): every device array below is a DevBuf member and goes with the object
// that holds it -- Segment destruction, a move assignment, segs.clear() -- so no list of frees exists anywhere.  The view structs of
// sweep.h that cross into a kernel are built from `.get()` per launch (abi_sweep.cpp pools_of) and never own.
// A segment of one kind leaves the groups of the other kinds empty.

// UniV3: everything a price change of the whole segment replaces.  univ3_build fills one; cfmm_update_reserves builds a fresh
// one per segment and moves it in.
struct UniV3State {
    DevBuf<double2> pg;
    DevBuf<double> cp;          // current_price alone (packed records)
    DevBuf<double2> cur_a, cur_b;
    DevBuf<double> cur_c;
    DevBuf<double2> curR;
    DevBuf<int4> walk;
    DevBuf<TickRec> ticks;      // walk lists (sweep.h TickRec)
    DevBuf<double> thr;         // drain thresholds, one per record
    DevBuf<uint4> head;         // per pool the first four thresholds of both walk lists as rounded-down floats (sweep.h UniV3Pools)
    int has_walk = 1;           // some pool has a tick beyond its current one
    // the walk lists of a pool that cfmm_pools_set_prices / _set_ticks moves are rewritten at the TAIL of ticks / thr
    // (abi_update.cpp): records in use (garbage of moved pools included) and allocated (thr: + 4 of read-ahead), and the host
    // copy of `walk` from which a compaction (compact_walks, update_kernels.h) lays the arrays out afresh
    int64_t tick_used = 0, tick_cap = 0;
    std::vector<int4> h_walk;
};

// N-coin kinds (KindInfo::ragged: CFMM_KIND_WEIGHTED, CFMM_KIND_CURVE): the coin-major columns and the segment's own trade
// arrays; such a segment has no rows in the two-coin trade buffers (trade_off is unused)
struct NCoinState {
    DevBuf<double> R;        // [n_coins][m] (sweep.h NCoinPools)
    DevBuf<double> q;        // [n_coins][m] the family's per-coin constant
    DevBuf<int32_t> tok;
    DevBuf<double2> glg;     // [m] {γ, log γ}
    DevBuf<double> par;      // the family's own column (KindInfo::par_per_pool doubles per pool)
    DevBuf<double> D, L;     // [n_coins][m] Δ, Λ of the latest materialising sweep
};

struct Segment : SegPlan {   // (SegPlan: the launch geometry, decided by ensure_geometry)
    int kind = 0;
    int64_t m = 0;
    int64_t n_ticks_total = 0;
    int fast_ok = 0; // every constant the sweep divides by / takes roots of lies in [2^-kFastExp, 2^kFastExp] (sweep.h)
    int n_coins = 2;
    // the two-coin kinds (UniV3: Ai, pk, gvals and the host copies only)
    DevBuf<double2> R, w;
    DevBuf<double> gamma;
    DevBuf<double> eta;      // geomean: η = w1/w2
    DevBuf<double2> lR;      // geomean: {Q1, Q2}, the v-independent constants of the log-space exponents (GeoMeanLogOps)
    DevBuf<int2> Ai;
    DevBuf<PackedFeeTok> pk;        // {i1 | i2 << 16, fee-table index} per pool, or empty (too many distinct fees / tokens)
    std::vector<double> gvals;      // the segment's distinct fees, in order of first appearance (index = PackedFeeTok::gidx)
    std::vector<int32_t> h_ai; // host copy of Ai: large-market mode (incidence build) and UniV3 segments
    // host copies of the pool constants that cfmm_pools_set_reserves prepares q / {Q1, Q2} from besides the new reserves:
    // GeometricMeanTwoCoin γ and η, weighted the normalised weights ([n_coins][m] like nc.par)
    std::vector<double> h_gamma, h_eta, h_par;
    // UniV3: the prepared state, and the pool definitions (update_reserves! moves current_price and re-derives the state from
    // them; cfmm_pools_set_ticks replaces single ladders: ladder_store.h).  n_ticks_total == lad.ticks_total().
    UniV3State u;
    std::vector<double> h_cp;
    LadderStore lad;
    NCoinState nc;
};

// What the library knows of a pool kind, in ONE place: the plan (launch_plan.cpp), the sweep (abi_sweep.cpp), the upload and
// the trade paths all read this table.  The device side of a kind is its Ops / Family struct in ops_two_coin.h, ops_univ3.h or sweep_ncoin.h.
struct KindInfo {
    const char* name;          // in error texts
    bool ragged;               // n_coins per pool: trades kept in the segment's own nc.D / nc.L, swept by sweep_ncoin
    bool fusable;              // may share a sweep_multi launch with its neighbours; false: always its own launch (the ragged
                               // kinds, and Solidly: a two-coin kind whose kernel is kept out of the fused launches)
    bool has_fast;             // has kernels on the fast arithmetic (Segment::fast_ok says whether a segment may use them)
    bool logv;                 // the sweep reads log v from LDS (SweepArgs::need_logv)
    bool exact_form;           // option "geomean_exact" swaps in the pow-based form, which has neither of the two above
    // relative cost of one pool evaluation in tenths of a ProductTwoCoin one: a constant or an option ("cost_geomean" /
    // "cost_univ3"; measured on config3 / mixed markets, see DESIGN), plus multi_tick_cost when the segment averages more
    // than 2 ticks per pool (a threshold scan + one more record).  Divides the blocks of a fused launch among its segments.
    int cost;
    int64_t PlanOpts::*cost_opt;
    int multi_tick_cost;
    bool par_coin_major;       // ragged kinds: the family's own column (NCoinPools::par) is [n_coins][m] (weights) or [m] pairs ({α, log β})
    // bytes one materialising sweep moves per pool: two-coin kinds the packed record + one 16-byte trade record (a lower bound
    // for multi-tick UniV3); ragged kinds per coin R, q, token (20 B) read and Δ, Λ (16 B) written, {γ, log γ}, par
    int64_t (*bytes_per_pool)(int n_coins, int has_walk);
    int64_t par_per_pool(int n_coins) const { return par_coin_major ? n_coins : 2; }
};
inline const KindInfo& kind_info(int kind)
{
    static const KindInfo table[] = {
        /* CFMM_KIND_PRODUCT  */ {"ProductTwoCoin", false, true, true, false, false, 10, nullptr, 0, false, [](int, int) -> int64_t { return 24 + 16; }},
        /* CFMM_KIND_GEOMEAN  */ {"GeometricMeanTwoCoin", false, true, true, true, true, 0, &PlanOpts::cost_geomean, 0, false, [](int, int) -> int64_t { return 48 + 16; }},
        /* CFMM_KIND_UNIV3    */ {"UniV3", false, true, true, false, false, 0, &PlanOpts::cost_univ3, 6, false, [](int, int walk) -> int64_t { return (walk ? 104 : 56) + 16; }},
        /* CFMM_KIND_WEIGHTED */ {"weighted", true, false, false, true, false, 0, nullptr, 0, true, [](int n, int) -> int64_t { return 36 * n + 16 + 8 * n; }},
        /* CFMM_KIND_CURVE    */ {"Curve", true, false, false, false, false, 0, nullptr, 0, false, [](int n, int) -> int64_t { return 36 * n + 16 + 8 * 2; }},
        /* CFMM_KIND_SOLIDLY  */ {"Solidly", false, false, false, false, false, 0, nullptr, 0, false, [](int, int) -> int64_t { return 24 + 16; }},
    };
    static_assert(CFMM_KIND_PRODUCT == 0 && CFMM_KIND_GEOMEAN == 1 && CFMM_KIND_UNIV3 == 2 && CFMM_KIND_WEIGHTED == 3 &&
                  CFMM_KIND_CURVE == 4 && CFMM_KIND_SOLIDLY == 5 && sizeof table / sizeof table[0] == 6, "one row per CFMM_KIND_*");
    return table[kind];
}
inline bool ragged_kind(int kind) { return kind_info(kind).ragged; }

struct Workers {
    // Multi-device parents: one persistent thread per shard >= 1 (shard 0 runs on the calling thread).  A call publishes
    // {v, materialize} and bumps `go`; workers spin briefly on it (an L-BFGS-B evaluation follows
    // the previous one within microseconds), then sleep on the condition variable.
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint64_t> go{0};
    std::atomic<int> pending{0};
    std::atomic<int> sleepers{0};
    std::atomic<bool> quit{false};
    const double* v = nullptr;
    bool materialize = false;
    std::vector<int> rc;
};

// The hand-over concerns of a context: each owns its resources (hostres.h, devbuf.h) and carries the few functions that
// touch them; all of it goes with the context.

// Zero-copy stage (abi_handover.cpp), pinned + device-mapped: [n] v in, [n+1] {Ψ, acc} out, padding to a 128-byte boundary,
// then the output granules (granule.h; 16 per fold block = 2 per column, columns padded to a multiple of 8; see fold_finish)
struct HostStage {
    PinnedBuf<double> buf;        // dev() null: no mapping, explicit copies
    int n = 0;
    size_t gran_off = 0;          // first output granule (doubles)
    size_t flag_off = 0;          // the sweeps' sticky report word (sweep.h kFlagWindow / kFlagGaveUp), its own 128-byte line
    uint64_t out_seq = 0;         // sequence number of the latest granule-delivering sweep
    bool last_host_out = false;   // the latest enqueue_sweep delivers {psi, acc} as granules (the caller polls them)
    double* out() const { return buf.host() + n; }   // the {Ψ, acc} slots
    int alloc(const cfmm_ctx* c, int n_tokens);
    unsigned long long take_flags(unsigned long long mask);
    bool granules_arrived(uint64_t seq);
    bool wait(uint64_t seq, long max_spins, double limit_s);
};

// Pre-armed evaluations of cfmm_route (sweep.h SweepArgs::arm_word): [n_pad] v, then the word, in FINE-GRAINED device
// memory that the host writes through the PCIe BAR (empty: no large BAR, or the self-check failed)
struct ArmState {
    DevBuf<double> buf;
    int n = 0, n_pad = 0;
    uint64_t seq = 0;             // sequence number of the latest armed launch
    bool pending = false;         // an armed launch is enqueued and has not been signalled or cancelled yet
    uint64_t tag = 0;             // output sequence number that launch will deliver
    const unsigned long long* word() const { return reinterpret_cast<const unsigned long long*>(buf.get() + n_pad); }
    void alloc(int device, int n_tokens, int n_padded);
    void write(const double* v, uint64_t word);
};

// Sparse pool-state updates (abi_update.cpp, cfmm_pools_set_*): pinned + device-mapped staging of the prepared records in
// 8-byte words, grown geometrically; `done` marks the end of the latest scatter launch (the staging is reused only after it)
struct UpdateStaging {
    PinnedBuf<unsigned long long> buf;
    Event done;
    bool busy = false;
    Event compact_ev[2];          // option "time_kernels": {start, stop} of the latest compact_walks launch
    int64_t compact_ns = 0;       // read-only option "compact_walks_ns": that launch's span
    int reserve(cfmm_ctx* c, size_t words);
};

// cfmm_select_trades (abi_trades.cpp, select_kernels.h): scratch, the device copy of the valuing prices and the compacted
// rows, grown on demand and kept for the next call; the scan delivers the count to one pinned, device-mapped word
struct SelectScratch {
    DevBuf<unsigned long long> mask;   // [blocks][kSelBlock / 64]
    DevBuf<int> counts;                // [blocks]
    DevBuf<long long> base;            // [blocks]
    DevBuf<double> v;                  // [n]
    DevBuf<long long> idx;             // [rows]
    DevBuf<double> D, L;               // [rows][n_coins]
    DevBuf<double> value;              // [rows]
    PinnedBuf<long long> total;
    Event ev[6];                       // option "time_kernels": {start, stop} per kernel
    int64_t ns[3] = {0, 0, 0};         // read-only options "select_flag_ns" / "select_scan_ns" / "select_emit_ns": the
                                       // latest timed call's kernel spans (emit: 0 when the call only counted)
};

// cfmm_quote and cfmm_quote_out (abi_quote.cpp, quote_kernels.h; one scratch for both directions): the device copies of one call's queries and answers and their pinned staging,
// grown on demand and kept for the next call -- proportional to the queries of the largest call, never to the pools.
// cfmm_quote_dev and cfmm_quote_out_dev use the two events only.
struct QuoteScratch {
    DevBuf<long long> idx;             // [count]
    DevBuf<int32_t> coins;             // [2][count] coin_in, coin_out
    DevBuf<double> amt, out;           // [count]
    PinnedBuf<unsigned long long> stage;   // 8-byte words: stage_layout.h QuoteStage
    EventPairs ev;                     // option "time_kernels": {start, stop} of the latest call's kernel
    int64_t ns = 0;                    // read-only option "quote_ns": that kernel's span
    bool dev_timed = false;            // the latest timed call was cfmm_quote_dev: its span is read when asked for
};

// The rig of the READ-ONLY path entries (cfmm_quote_path(_out), cfmm_size_path, cfmm_split_paths(_out) and their _dev forms;
// the functions: path_rig.h): the segment table (sweep.h PathSeg) on the device and the entry's ONE pinned staging buffer, whose
// first column is the table's host copy.  The table is rebuilt and uploaded on every call; `done`, recorded behind each
// call's kernel, guards the staging and the table against the call before (the _dev entries do not wait).
struct PathRig {
    DevBuf<PathSeg> table;             // [segments]
    PinnedBuf<unsigned long long> stage;   // 8-byte words: the entry's layout of stage_layout.h
    Event done;                        // behind the latest call's kernel
    bool in_flight = false;
    int wait_previous(cfmm_ctx* c);
    template <class Layout>
    int upload_table(cfmm_ctx* c, const Layout& lay, int32_t& nrec_out);   // Layout: the entry's of stage_layout.h
    template <class Launch>
    int launch(cfmm_ctx* c, EventPairs& ev, const char* what, const Launch& go);
};
// ... of an entry with a span of its own ("size_ns", "split_ns") and a launch count
struct TimedPathRig : PathRig {
    EventPairs ev;                     // option "time_kernels": {start, stop} of the latest call's kernel
    int64_t ns = 0;                    // that kernel's span (a parent: the sum of its rounds' "quote_ns")
    bool dev_timed = false;            // the latest timed call was the _dev entry: its span is read when asked for
    int64_t launches = 0;              // kernel launches of the latest call (1; a parent: its cfmm_quote_path calls)
    int read_ns(cfmm_ctx* c, int64_t* value);
};

// cfmm_quote_path and cfmm_quote_path_out (abi_quote_path.cpp, quote_path_kernels.h; one scratch for both directions): the rig
// and the device copies of one call's paths, amounts, answers and optional hop amounts -- proportional to count x max_hops
// (and the number of segments), never to the pools.  The kernel's span goes to QuoteScratch's events and "quote_ns".
struct PathScratch : PathRig {         // (stage: stage_layout.h PathStage)
    DevBuf<int32_t> hop_i32;           // [1 + 3*max_hops][count]: n_hops, then hop_seg, hop_coin_in, hop_coin_out
    DevBuf<long long> hop_row;         // [max_hops][count]
    DevBuf<double> given, answer;      // [count]
    DevBuf<double> hops;               // [max_hops][count]
};

// cfmm_quote_rate and cfmm_quote_path_rate (abi_rate.cpp, rate_kernels.h): the query columns, the staging, the table and the rig
// are QuoteScratch's and PathScratch's (a call of either entry ends synchronised); what is kept here is the device copy of the
// two answers per query / path and per hop, and the span of the latest call's kernel -- proportional to the queries, never
// to the pools.
struct RateScratch {
    DevBuf<double> out;                // [2][count] amount_out, rate
    DevBuf<double> hops;               // [2][max_hops][count] hop_out, hop_rate
    EventPairs ev;                     // option "time_kernels": {start, stop} of the latest call's kernel
    int64_t ns = 0;                    // read-only option "rate_ns": that kernel's span
    bool dev_timed = false;            // the latest timed call was a _dev entry: its span is read when asked for
};

// cfmm_quote_to_rate (abi_limit.cpp, to_rate_kernels.h): the query columns and the staging are QuoteScratch's (the limits travel
// in its amounts); kept here: the device copy of the two answers per query and the span of the latest call's kernel.
struct ToRateScratch {
    DevBuf<double> out;                // [2][count] amount_in, amount_out
    EventPairs ev;                     // option "time_kernels": {start, stop} of the latest call's kernel
    int64_t ns = 0;                    // read-only option "limit_ns": that kernel's span
    bool dev_timed = false;            // the latest timed call was the _dev entry: its span is read when asked for
};

// cfmm_swap and cfmm_swap_out (abi_swap.cpp, swap_kernels.h, swap_out_kernels.h; one scratch for both directions): the
// device copies of one call's swaps -- in WAVE order (swap_waves.h) -- their answers, the UniV3 landing prices and the pinned
// staging of all of them, grown on demand and kept for the next call -- proportional to the swaps of the largest call, never
// to the pools.
struct SwapScratch {
    DevBuf<long long> idx;             // [count]
    DevBuf<int32_t> coins;             // [2][count] coin_in, coin_out
    DevBuf<double> amt, out, price;    // [count]; price: UniV3 segments only
    DevBuf<double> limit;              // [count] cfmm_swap_out: max_amount_in, where given
    DevBuf<int32_t> status;            // [count] cfmm_swap_out: CFMM_SWAP_*; cfmm_swap_limit: CFMM_LIMIT_*
    DevBuf<double> used;               // [count] cfmm_swap_limit: amount_used
    DevBuf<int> left;                  // [1] a new reserve left the window of the fast arithmetic (update_two_coin's flag)
    PinnedBuf<unsigned long long> stage;   // 8-byte words: stage_layout.h SwapStage
    EventPairs ev;                     // option "time_kernels": {start, stop} per wave of the latest call
    int64_t ns = 0;                    // read-only option "swap_ns": the sum of that call's kernel spans
    int64_t refused = 0;               // read-only option "swap_refused": swaps of the latest call that were not applied
    int64_t launches = 0;              // read-only option "swap_launches": kernel launches (waves) of the latest call
};

// cfmm_swap_path(_out) and cfmm_swap_order(_out) (abi_swap_path.cpp swap_paths_run; swap_path_kernels.h, swap_order_kernels.h;
// ONE scratch for the four: each call ends synchronised, so nothing here is guarded against the call before): the device
// copies of one call's paths and orders, both in WAVE order (swap_path_waves.h), the limits, answers, hop amounts, UniV3
// landing prices and statuses, the segment table (sweep.h SwapPathSeg, rebuilt per call), one window flag per segment and ONE
// pinned staging buffer for all of them -- proportional to the orders and to n_paths x max_hops (and the number of
// segments), never to the pools.  The path entries have no orders: the tails marked "orders" are empty and the limits are the
// paths'.  The spans, the refusals and the waves go to SwapScratch's "swap_ns" / "swap_refused" / "swap_launches".
struct SwapPathScratch {
    DevBuf<SwapPathSeg> table;         // [segments]
    DevBuf<int32_t> hop_i32;           // [1 + 3*max_hops][n_paths]: n_hops, then hop_seg, hop_coin_in, hop_coin_out
    DevBuf<long long> i64;             // [max_hops][n_paths] hop_row, then (orders) [count + 1] order_first
    DevBuf<double> amt;                // [n_paths] the given amounts, then the limits ([count] of the orders, else [n_paths])
    DevBuf<double> out;                // [n_paths] the paths' answers, then (orders) [count] the totals
    DevBuf<double> hops, price;        // [max_hops][n_paths]
    DevBuf<int32_t> status;            // [n_paths] the paths' statuses, then (orders) [count] status
    DevBuf<int> left;                  // [segments] a new reserve of the segment left the window of the fast arithmetic
    PinnedBuf<unsigned long long> stage;   // 8-byte words: stage_layout.h SwapPathStage
    EventPairs ev;                     // option "time_kernels": {start, stop} per wave of the latest call
    PathPoolTable pools;               // the wave planner's table (swap_path_waves.h), host memory kept between calls
};

// cfmm_find_path (abi_find_path.cpp, find_path_kernels.h): the layers of the search -- the one array of the path features that
// is proportional to n_tokens: (max_hops + 1) x queries of a chunk x n_tokens words, bounded by kFindScratchBudget
// (find_checks.h) -- the claimed edges, the device copies of one call's queries and answers, the segment table (sweep.h
// FindSeg, rebuilt per call) and ONE pinned staging buffer, all grown on demand and kept for the next call.  The call ends
// synchronised, so nothing here is guarded against the call before.  cfmm_find_path_out uses the same scratch with the roles of
// the amounts exchanged (best: the layers of its min-search, all ones = unreached; edge[k]: hop k in path order); the read-only
// options describe the latest call of either entry.  cfmm_find_disjoint_paths (include/cfmm_amd_find_disjoint.h) uses it too, its
// outputs max_paths times as large (the layout: abi_find_path.cpp find_disjoint), plus the ban rows.
struct FindScratch {
    DevBuf<FindSeg> table;             // [segments]
    DevBuf<unsigned long long> best;   // [max_hops + 1][chunk][n_tokens]
    DevBuf<unsigned long long> edge;   // [max_hops][chunk]
    DevBuf<int32_t> i32;               // [4][count] token_in, token_out, n_hops, status; [3][max_hops][count] hop_seg, hop_coin_in,
                                       // hop_coin_out; [2][chunk] the hops of the answer, the walk's target token
    DevBuf<long long> hop_row;         // [max_hops][count]
    DevBuf<double> amt;                // [2][count] amount_in, amount_out
    DevBuf<unsigned long long> ban;    // cfmm_find_disjoint_paths: [chunk][ceil(pools / 64)] the pools absent for each query, cleared per chunk
    PinnedBuf<unsigned long long> stage;   // 8-byte words: stage_layout.h FindStage / FindDisjointStage
    EventPairs ev;                     // option "time_kernels": {start, stop} per launch of the latest call
    int64_t relax_ns = 0, walk_ns = 0; // read-only options "find_relax_ns" / "find_walk_ns": the sums of that call's find_relax spans
                                       // and of its find_claim + find_advance spans
    int64_t launches = 0;              // read-only option "find_launches": kernel launches of the latest call
    // the same spans layer by layer, summed over the call's chunks: read-only options "find_relax_ns_<h>", "find_claim_ns_<h>",
    // "find_advance_ns_<h>", h = 1 .. CFMM_MAX_PATH_HOPS (0 for a layer the call did not have)
    int64_t layer_ns[3][CFMM_MAX_PATH_HOPS] = {};
    // ... and round by round (cfmm_find_disjoint_paths; the other entries have one round): read-only options
    // "find_round_relax_ns_<r>" / "find_round_walk_ns_<r>", r = 1 .. CFMM_MAX_SPLIT_PATHS
    int64_t round_ns[2][CFMM_MAX_SPLIT_PATHS] = {};
};

// cfmm_size_path (abi_size_path.cpp, size_path_kernels.h): the rig (read-only options "size_ns" / "size_launches") and the
// device copies of one call's paths, limits, values and answers -- proportional to count x max_hops (and the number of
// segments), never to the pools.  A multi-device parent uses none of the device arrays: its search runs on the host
// (size_grid.h) over cfmm_quote_path.
struct SizeScratch : TimedPathRig {    // (stage: stage_layout.h SizeStage)
    DevBuf<int32_t> hop_i32;           // [1 + 3*max_hops][count]: n_hops, then hop_seg, hop_coin_in, hop_coin_out
    DevBuf<long long> hop_row;         // [max_hops][count]
    DevBuf<double> in;                 // [3][count] max_amount_in, value_in, value_out
    DevBuf<double> out;                // [3][count] amount_in, amount_out, gain
    DevBuf<int32_t> status;            // [count]
};

// cfmm_split_paths and cfmm_split_paths_out (abi_split_paths.cpp, split_paths_kernels.h, split_paths_out_kernels.h): the rig
// (read-only options "split_ns" / "split_launches") and the device copies of one call's orders, paths and answers, proportional
// to the orders and to n_paths x max_hops, never to the pools.  A multi-device parent uses none of the device arrays: its
// search runs on the host (split_search.h) over cfmm_quote_path / cfmm_quote_path_out.
struct SplitScratch : TimedPathRig {   // (stage: stage_layout.h SplitStage)
    DevBuf<int32_t> hop_i32;           // [1 + 3*max_hops][n_paths]: n_hops, then hop_seg, hop_coin_in, hop_coin_out
    DevBuf<long long> i64;             // [max_hops][n_paths] hop_row, then [count + 1] order_first
    DevBuf<double> amount;             // [count]
    DevBuf<double> out;                // [2][n_paths] path_amount_in, path_amount_out, then [count] total_out
    DevBuf<int32_t> status;            // [count]
};

// The launch-invariant descriptors of the sweep launches (sweep.h SweepDesc; launch_plan.h build_sweep_desc) on the device,
// one after the other BEHIND the launches' fee tables in cfmm_ctx::d_gtab (ensure_geometry sizes that array for both: what
// a launch reads and no evaluation changes is one device array): rebuilt by ensure_desc (abi_sweep.cpp) when
// cfmm_ctx::desc_dirty is set or a resource of the library has been created or released since (resource_epoch, devbuf.h),
// copied from the pinned staging in stream order.  Every device of a multi-device context owns one (its child context's).
struct SweepDescStore {
    size_t base = 0, bytes = 0;      // where the descriptors start in d_gtab (bytes), and their size
    PinnedBuf<unsigned char> stage;
    Event uploaded;                  // behind the latest copy stage -> device: the staging is rewritten only after it
    bool in_flight = false;
    uint64_t epoch = 0;              // resource_epoch() when the descriptors were built
    std::vector<size_t> off;         // [groups] where each launch group's descriptor starts (kNoDesc: it takes none)
    std::vector<SweepDesc> heads;    // [groups] host copies of the heads: LDS sizes, the arithmetic, sweep_ncoin's arguments
    unsigned char* dev(const cfmm_ctx* c) const;
};

// Kernel timing (option "time_kernels"): a pool of events, the {start, stop} pairs not yet read, the totals
struct KernelTimer {
    std::vector<Event> pool;
    size_t used = 0;
    struct Pending { hipEvent_t a, b; int what; };
    std::vector<Pending> pending;
    int64_t sweep_n = 0, reduce_n = 0;
    double sweep_ms = 0, reduce_ms = 0;
    void take_events(hipEvent_t& a, hipEvent_t& b);   // a start / stop pair for one timed launch (both null when none could be had)
    int harvest(cfmm_ctx* c, int64_t* sweep_launches, double* sweep_ms_out, int64_t* reduce_launches, double* reduce_ms_out);
};

} // namespace cfmm

struct cfmm_ctx {
    int device = 0;
    int n = 0;
    int n_pad = 0;
    // FIRST among the members that own a HIP resource: members go in reverse order, so the context's own stream is
    // released after every DevBuf, pinned buffer and event below
    cfmm::Stream own_stream;
    hipStream_t stream = nullptr;
    std::vector<cfmm::Segment> segs;
    std::vector<cfmm::Group> groups;
    int64_t m_total = 0;
    int64_t trade_rows = 0;       // rows of the two-coin trade buffers (pools of the two-coin segments; weighted segments keep their own)
    int64_t flat_total = 0;       // Σ over segments of m × coins: the length of each ragged trade array (cfmm_trades_len)
    bool any_ragged = false;      // some segment is ragged (KindInfo::ragged: weighted, Curve): its trades are ragged
    int64_t touched_bytes = 0;    // what one materialising sweep moves by construction (packed layout; ensure_geometry): decides "stream_stores" = auto
    int64_t rows_total = 0;

    // device buffers: DevBufs, grown on demand (DevBuf::grow: the old contents go) and released with the context
    cfmm::DevBuf<double> d_v;        // [n]
    cfmm::DevBuf<double> d_out;      // [n+1]
    cfmm::DevBuf<double> d_partials; // [rows][row_width]: n+1 columns, rows padded to 128 bytes
    // trade buffers, one size each.  Compact layout (option "compact_trades", default): d_delta holds ONE 16-byte
    // record per pool, d_lambda / d_over the four values of the rare pools that trade in both directions (sweep.h
    // SweepArgs); plain layout: d_delta = {Δ₁, Δ₂}, d_lambda = {Λ₁, Λ₂}.  d_xdelta / d_xlambda: expanded copies, for
    // cfmm_trades_dev and the trade download.
    cfmm::DevBuf<double2> d_delta, d_lambda, d_over;
    cfmm::DevBuf<double2> d_xdelta, d_xlambda;
    bool x_valid = false;         // d_xdelta / d_xlambda hold the expansion of the trades currently on the device
    int trades_compact = 0;       // layout of the trades currently on the device
    cfmm::TradeStaging tstage;
    // large-market mode (n > kMaxLdsTokens): token -> (pool, side) incidence and flow scratch
    cfmm::DevBuf<double2> d_flow;       // [m_total] {Λ₁−Δ₁, Λ₂−Δ₂}
    cfmm::DevBuf<int> d_entries;        // [2·m_total] flat flow indices grouped by token
    cfmm::DevBuf<int2> d_chunks;        // [n_chunks] {begin, end} into d_entries
    cfmm::DevBuf<int> d_tok_chunk_off;  // [n+1]
    cfmm::DevBuf<double> d_chunk_sums;  // [n_chunks]
    int n_chunks = 0;
    // sharded operation (cfmm_set_peers): the fold launch of every sweep also gathers the peers' {Ψ, acc} over xGMI
    // (reduce_gather), so eval / find_arb / route return GLOBAL {Ψ, acc}
    std::vector<uint64_t> peers;  // device addresses of all ranks' symmetric buffers
    int peer_rank = 0;
    uint64_t peer_seq = 0;
    long long peer_timeout_ticks = 3000000000ll;   // 30 s of wall_clock64() at 100 MHz (CFMM_AMD_PEER_TIMEOUT_S)
    // sharded operation through RCCL (cfmm_set_rccl_comm / cfmm_rccl_init_rank, abi_rccl.cpp): every sweep's fold is followed,
    // in-stream, by ncclAllReduce(d_out, n + 1 doubles) -- same contract as `peers`, one exchange at a time
    void* rccl_comm = nullptr;    // ncclComm_t
    bool rccl_owned = false;      // created by cfmm_rccl_init_rank: destroyed with the context
    cfmm::HostStage stage;
    cfmm::DevBuf<double> d_gtab;  // [groups][kMaxFeeTable] fee tables of the launches (packed pool records), then their descriptors (desc)
    cfmm::ArmState arm;
    std::vector<double> last_out; // psi..., acc of the latest host-pointer sweep
    std::vector<double> trade_v;  // v of the latest MATERIALISING host-pointer sweep (empty: none / device-pointer sweep)
    bool have_out = false;
    bool have_trades = false;
    bool geometry_dirty = true;
    // the sweep descriptors copy something that has changed.  Set wherever geometry_dirty is, by every cfmm_set_option, by
    // cfmm_set_peers and cfmm_set_stream, and wherever an array a descriptor points to is swapped for another (UniV3 state
    // replaced or regrown, tick compaction); ensure_desc also compares resource_epoch
    bool desc_dirty = true;
    cfmm::SweepDescStore desc;

    // options (cfmm_set_option)
    cfmm::PlanOpts geo;          // the options the launch geometry depends on (launch_plan.h)
    int64_t opt_time_kernels = 0;
    int64_t opt_zero_copy = 1;     // 1: host-pointer calls read v / receive Ψ through mapped pinned memory
    int64_t opt_compact_trades = 1; // 1: a materialising sweep writes one 16-byte trade record per pool (+ overflow rows)
    int64_t opt_alternate = 1;     // 1: consecutive sweeps walk the tiles in alternating directions (L2 reuse across sweeps)
    int64_t opt_fast_math = 1;     // 1: division / square root without range scaffolding where operands are inside the window (same bits)
    int64_t opt_armed = 1;         // 1: cfmm_route enqueues evaluation k+1 while evaluation k runs (see abi_handover.cpp)
    int64_t opt_arm_timeout_ms = 2000; // bound of that wait
    int64_t opt_host_flag = 1;     // 1: zero-copy host-pointer sweeps deliver {Ψ, acc} as self-validating granules that the caller
                                   //    polls, instead of waiting for the stream (saves the end-of-kernel + signal path)
    int64_t opt_stop_in_noise = 0; // cfmm_route: 1 = end the run when a line-search trial point sits on the rounding-noise floor
                                   //    (LbfgsbOptions::stop_in_noise; fewer evaluations, departs from L-BFGS-B 3.0); 0 = reference behaviour
    int64_t opt_multi_threads = 1;
    int64_t opt_stream_stores = 0; // trade-record stores: 0 = auto (non-temporal when one sweep touches more than the 256 MiB Infinity Cache,
                                   //    i.e. the pool state cannot stay cache-resident between sweeps; write-through otherwise), 1 = always
                                   //    write-through, 2 = always non-temporal (a caller that rotates over many markets says so)
    int64_t opt_find_lds = 1;      // 1: cfmm_find_path's layer launches fold their candidates into a per-block LDS copy of the layer rows
                                   //    first, where n_tokens lets one fit (find_path_kernels.h find_relax<., true>); 0: every candidate
                                   //    goes to global memory (the A/B of scripts/find_path_times.py; the same bits either way)
    int64_t opt_size_max_blocks = cfmm::kSizeMaxBlocks; // cfmm_size_path: the most blocks of its launch (>= 1; its wavefronts stride over the
                                   //    paths, the same bits at any value: a measurement and test switch)
    int64_t opt_split_max_blocks = cfmm::kSplitMaxBlocks; // cfmm_split_paths: the same switch of its launch (its wavefronts stride over the orders)
    int64_t opt_univ3_heads = 1;   // 1: multi-tick UniV3 walks decide their first four list ticks from the per-pool float threshold heads
    int64_t opt_lean_kernels = 1;  // 1: a launch in the default configuration takes the lean form of its kernel (launch_plan.h lean_launch:
                                   //    the same bits with fewer instructions per tile); 0: always the general kernels (A/B, tests)
    int64_t lean_launches = 0;     // read-only option "lean_launches": sweep launches of this context that took a lean kernel
    int64_t opt_dev_prices_in_window = 0; // 1 = the CALLER vouches that the prices of device-pointer sweeps lie in [2^-kFastExp, 2^kFastExp]
                                     //    (what the host checks itself for host-pointer calls): cfmm_sweep_dev launches the fast kernels
                                     //    instead of the ones that carry both arithmetics; every block still checks what it stages and
                                     //    poisons its row (NaN in {psi, acc}: an error, never a wrong number) when the promise is broken
    int64_t opt_debug_stall_ms = 0; // test hook, reachable only in libcfmm_amd_hooks.so (-DCFMM_TEST_HOOKS: the option key and the stall
                                    //    exist there alone; the FIELD is unconditional so that every translation unit sees one layout)
    uint64_t sweep_count = 0;

    cfmm::UpdateStaging upd;
    int64_t pool_update_regrows = 0;   // read-only option "pool_update_regrows": compactions + regrows of UniV3 tick arrays
    cfmm::SelectScratch sel;
    cfmm::QuoteScratch quote;
    cfmm::PathScratch path;
    cfmm::RateScratch rate;
    cfmm::ToRateScratch to_rate;
    cfmm::SwapScratch swap;
    cfmm::SwapPathScratch swap_path;
    cfmm::FindScratch find;
    cfmm::SizeScratch size;
    cfmm::SplitScratch split;
    cfmm::KernelTimer timer;

    // single-process multi-device parent (cfmm_ctx_create_multi): shards non-empty, no device state of its own
    std::vector<cfmm_ctx*> shards;
    struct ParentSeg { int kind; int64_t m; int64_t trade_off; int n_coins; int64_t flat_off; };   // flat_off: see Segment
    std::vector<ParentSeg> psegs;          // one per cfmm_pools_add_* call with m > 0
    std::unique_ptr<cfmm::Workers> workers;
    bool shards_distinct = true;           // no two shards share a device (pre-armed evaluations need that)

    // cfmm_swap_order / cfmm_swap_order_out.  (Behind everything above, so that every member the sweep's host path reads stands
    // where it stood before these two came.)
    int64_t opt_order_max_blocks = cfmm::kOrderMaxBlocks; // the most blocks of their launches (>= 1; the wavefronts stride over a wave's
                                   //    orders, the same bits at any value: a measurement and test switch, as "split_max_blocks")

    mutable std::string err = "";
};

namespace cfmm {

extern thread_local std::string g_create_error;

#define HIP_TRY(ctx, expr)                                                                            \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return ::cfmm::fail(ctx, CFMM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));    \
    } while (0)

#define CFMM_SINGLE_ONLY(c, what)                                                                     \
    if (!(c)->shards.empty() || (c)->device < 0)                                                      \
        return ::cfmm::fail(c, CFMM_ERR_UNSUPPORTED, what " is not available on a multi-device context (host-pointer calls only)")

inline bool global_bins(const cfmm_ctx* c) { return global_bins(c->n); }
inline unsigned char* SweepDescStore::dev(const cfmm_ctx* c) const { return reinterpret_cast<unsigned char*>(c->d_gtab.get()) + base; }
inline int row_width(const cfmm_ctx* c) { return global_bins(c) ? 1 : row_pitch_of(c->n + 1); }   // doubles between partial rows
inline bool is_parent(const cfmm_ctx* c) { return !c->shards.empty() || c->device < 0; }

// abi_upload.cpp
int univ3_build(cfmm_ctx* c, UniV3State& u, int& fast_ok, int64_t m, const double* current_price, const double* gamma, const int32_t* Ai,
                const int64_t* tick_off, const double* lower_ticks, const double* liquidity);

// abi_sweep.cpp
int ensure_geometry(cfmm_ctx* c);
constexpr int kPricesUnknown = 0, kPricesInWindow = 1, kPricesOutside = 2;
int enqueue_sweep(cfmm_ctx* c, const double* d_v, double* d_out, bool materialize, bool want_host_out = false,
                  uint64_t arm_seq = 0, int price_window = kPricesUnknown);

// abi_handover.cpp
bool prices_in_fast_window(const double* v, int n);
int check_prices(cfmm_ctx* c, const double* v);
int host_sweep_begin(cfmm_ctx* c, const double* v, bool materialize);
int host_sweep_end(cfmm_ctx* c);
int single_host_sweep(cfmm_ctx* c, const double* v, bool materialize);
int host_sweep(cfmm_ctx* c, const double* v, bool materialize);   // single device or parent
bool can_arm(cfmm_ctx* c);
void armed_cancel(cfmm_ctx* c);
int armed_eval(cfmm_ctx* c, const double* v, bool* lost_out);      // single device or parent

// abi_multi.cpp (shard_range: shard_split.h)
int multi_host_sweep(cfmm_ctx* c, const double* v, bool materialize);
int multi_add(cfmm_ctx* c, int kind, int64_t m, const std::function<int(cfmm_ctx*, int64_t, int64_t)>& add, int n_coins = 2);
int child_segment(const cfmm_ctx* c, int pseg, int d);
int multi_get_trades_range(cfmm_ctx* c, int32_t seg, int64_t first, int64_t count, double* Delta, double* Lambda);
int multi_select_trades(cfmm_ctx* c, int32_t seg, const double* v, double min_value, int64_t capacity, int64_t* count, int64_t* idx,
                        double* Delta, double* Lambda, double* value);

// abi_quote.cpp
int quote_ns(cfmm_ctx* c, int64_t* value);
// cfmm_quote's checks of one call under the name `who` (`given`: how the messages spell the amount), before anything is
// enqueued: the segment and count, then every query.  n_segs, kind, m, nc: the segment as the context (single or parent) sees it.
int check_quote_seg(cfmm_ctx* c, const char* who, int32_t seg, int64_t count, int64_t n_segs);
int check_quote_queries(cfmm_ctx* c, const char* who, const char* given_name, int kind, int64_t m, int nc, int64_t count,
                        const int64_t* idx, const int32_t* coin_in, const int32_t* coin_out, const double* given, const double* answer);

// abi_rate.cpp
int rate_ns(cfmm_ctx* c, int64_t* value);
// abi_limit.cpp
int limit_ns(cfmm_ctx* c, int64_t* value);

// abi_update.cpp
// cfmm_pools_set_prices' apply path on rows that are distinct, ascending and already checked (each price finite, > 0 and not
// above the row's first tick): apply_univ3 for the records prepared on the host, univ3_make_room, one scatter; h_cp follows.
// Enqueued on the context's stream; invalidates nothing by itself (the caller does).
int univ3_move_prices(cfmm_ctx* c, Segment& s, const std::vector<int64_t>& rows, const double* price);

// abi_swap.cpp
// the trades and outputs on the device describe the market before the swaps: what cfmm_pools_set_* invalidates
void swap_invalidate(cfmm_ctx* c);

// abi_swap_path.cpp
// One checked call of cfmm_swap_path(_out) or cfmm_swap_order(_out) on a single-device context, count > 0: the plan, the
// staging, one launch per wave, the UniV3 moves between waves, the answers back in the caller's order.
struct SwapPathCall {
    const char* what;              // "swap path" / "swap order": the launch error's text
    int64_t orders;                // 0: the path entries -- every path is applied on its own, `limit` has one entry per path
    const int64_t* order_first;    // [orders + 1], null without orders
    int64_t n_paths;
    int32_t max_hops;
    HopCols hop;
    const double *given, *limit;   // limit: null = none
    double *answer, *hop_ans;      // [n_paths]; [max_hops][n_paths] or null
    int32_t* path_status;          // [n_paths] or null
    double* total;                 // [orders]
    int32_t* status;               // [orders]
};
// `launch`: one wave.  a.p is a SwapPathArgs for the wave's paths (the path entries; a.orders == 0) or for all paths of the call
// with the wave's orders beside it (sweep.h SwapOrderArgs).
using SwapWaveLaunch = hipError_t (*)(const cfmm_ctx* c, bool exact_out, const SwapOrderArgs& a, hipEvent_t e0, hipEvent_t e1);
int swap_paths_run(cfmm_ctx* c, bool exact_out, const SwapPathCall& q, SwapWaveLaunch launch);

// abi_rccl.cpp
int rccl_all_reduce_out(cfmm_ctx* c, double* d_out);
void rccl_release(cfmm_ctx* c);

} // namespace cfmm
