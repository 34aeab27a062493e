/*
 * cfmm_amd.h -- C ABI of libcfmm_amd.so: the MI355X (gfx950) implementation of
 * CFMMRouter.jl's per-CFMM arbitrage sweep and the reductions route! consumes.
 *
 * The reference has no FFI seam (it is one Julia module); this header IS the seam a
 * maintainer binds with `ccall` (julia/CFMMRouterAMD.jl).  Each entry
 * point names the reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C, no exceptions: every call returns CFMM_OK (0) or a negative error code;
 *     cfmm_last_error() returns the message.  (Reference: ArgumentError from the
 *     constructors src/cfmms.jl:77-78, src/objectives.jl:54,97 -- nothing else.)
 *   - all values are IEEE binary64, computed in binary64 on the device.
 *   - token indices are 0-based int32 on this side (reference: 1-based Int64,
 *     src/cfmms.jl:10,16); the binding subtracts 1 when packing.
 *   - "pair" arrays are [m][2] row-major: R = {R1,R2}, Ai = {i1,i2}, w = {w1,w2},
 *     Delta = {D1,D2}, Lambda = {L1,L2} -- the reference's per-pool 2-vectors, contiguous.
 *   - host pointers are only read/written during the call; the library copies.
 *   - a cfmm_ctx is bound to one device and is not re-entrant; distinct contexts are
 *     independent.  Host-pointer calls are synchronous; *_dev calls are asynchronous on
 *     the context's stream.
 *   - pools are stored in SEGMENTS (one per cfmm_pools_add_* call with m > 0, each homogeneous
 *     in pool family; an empty batch is accepted and ignored).  Trade arrays are laid out segment after segment in call order, so a
 *     router whose cfmms vector is grouped by family keeps the reference's pool order.
 */
#ifndef CFMM_AMD_H
#define CFMM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFMM_OK 0
#define CFMM_ERR_INVALID_ARG (-1) /* bad pointer / size / pool data (the reference's ArgumentError) */
#define CFMM_ERR_HIP (-2)         /* a HIP runtime call failed; message carries hipGetErrorString */
#define CFMM_ERR_STATE (-3)       /* call sequence error (e.g. netflows before any sweep) */
#define CFMM_ERR_UNSUPPORTED (-4) /* valid request outside the implemented envelope */

#define CFMM_KIND_PRODUCT 0 /* ProductTwoCoin        src/cfmms.jl:101-140 */
#define CFMM_KIND_GEOMEAN 1 /* GeometricMeanTwoCoin  src/cfmms.jl:152-196 */
#define CFMM_KIND_UNIV3 2   /* UniV3/BoundedProduct  src/cfmms.jl:226-395 */
#define CFMM_KIND_WEIGHTED 3 /* GeometricMean / Product with 2..8 coins  src/cfmms.jl:57-64 (no find_arb! there) */
#define CFMM_KIND_CURVE 4    /* Curve (StableSwap) with 2..8 coins       src/cfmms.jl:66-70 (no find_arb! there) */
#define CFMM_KIND_SOLIDLY 5  /* Solidly-style stable pair, phi = x^3 y + x y^3 (no such pool in the reference) */

typedef struct cfmm_ctx cfmm_ctx;

/* ---- lifetime ------------------------------------------------------------------------ */

/* Router(objective, cfmms, n_tokens) -- src/router.jl:18-36: the device-side half of the
 * Router (pool store, trade buffers, v).  device_id is a HIP ordinal. */
int cfmm_ctx_create(int device_id, int32_t n_tokens, cfmm_ctx** out);
void cfmm_ctx_destroy(cfmm_ctx* ctx);

/* The same Router sharded over the GPUs of one node from ONE host thread / process:
 * the parallel axis of src/router.jl:39 (`Threads.@threads for i in 1:length(r.Δs)`) split into
 * n_devices contiguous blocks.  Every cfmm_pools_add_* batch is divided into contiguous blocks over
 * the devices (no pool is replicated); every host-pointer sweep (cfmm_find_arb, cfmm_eval, and
 * therefore cfmm_route: ONE L-BFGS-B drives all shards) stages v on every device, runs the shard
 * sweeps concurrently and adds the shards' {psi, acc} in device-list order on the host -- v comes
 * from the host and psi returns to it on every evaluation, so the all-reduce of a sharded route! is
 * n_devices * (n_tokens + 1) host additions; no peer mapping, no IPC, no RCCL, no torch.  Results
 * are independent of the option "multi_threads" (1, default: one host worker thread per device
 * launches and waits; 0: the calling thread launches on every device, then waits for each).
 * A device id may be listed more than once (several shards on one GPU: used by the 1-GPU tests).
 * Trade arrays keep the single-device layout (segment after segment, pools in upload order).
 * Not available on such a context: cfmm_set_stream, cfmm_sweep_dev, cfmm_trades_dev, cfmm_set_peers
 * (CFMM_ERR_UNSUPPORTED), and n_tokens > 8192.  For one process PER GPU use cfmm_ctx_create +
 * cfmm_set_peers / RCCL instead (cfmmrouter.jl_amd/dist.py). */
int cfmm_ctx_create_multi(int32_t n_devices, const int32_t* device_ids, int32_t n_tokens, cfmm_ctx** out);
int32_t cfmm_device_count(const cfmm_ctx* ctx); /* shards of the context (1 for cfmm_ctx_create) */

/* Message of the last failing call on ctx (ctx == NULL: last failing cfmm_ctx_create on
 * this thread).  Never NULL; valid until the next call on the same ctx/thread. */
const char* cfmm_last_error(const cfmm_ctx* ctx);
const char* cfmm_version(void);

/* Launch on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * context's own non-blocking stream.  NULL means HIP's default (null) stream -- exactly the
 * handle given is used.  cfmm_reset_stream returns to the context's own stream. */
int cfmm_set_stream(cfmm_ctx* ctx, void* hip_stream);
int cfmm_reset_stream(cfmm_ctx* ctx);

/* Options (int64 values; unknown keys are CFMM_ERR_INVALID_ARG).  Results never depend on the tuning knobs beyond
 * summation-order rounding of psi / acc; trades are bit-identical under all of them.
 *   launch geometry   "block" (0 = auto | 512 | 1024 threads), "max_grid" (0 = auto), "bin_copies" (0 = auto, 1 = one
 *                     LDS netflow copy per block, 2 = one per wavefront), "fuse_segments" (default 1: all pool families
 *                     swept by one launch; 0: one launch per segment), "cost_geomean" / "cost_univ3" (cost of one
 *                     evaluation in tenths of a ProductTwoCoin one: how a fused launch divides its blocks; 10 / 10)
 *   data layout       "pack" (default 1: sweeps read an 8-byte {token pair, fee-table index} record instead of gamma +
 *                     Ai when a launch's distinct fees fit a 256-entry table), "compact_trades" (default 1: a
 *                     materialising sweep stores ONE 16-byte record per pool -- {+Delta1, Lambda2} or {-Delta2,
 *                     Lambda1}, a two-coin trade has one direction -- plus overflow rows for pools whose four values
 *                     do not fit that form; cfmm_get_trades* / cfmm_trades_dev return the reference's rows bit for bit),
 *                     "stream_stores" (trade records leave through 0 = auto: non-temporal stores when one sweep touches more
 *                     than the 256 MiB Infinity Cache -- the pool state then comes from HBM on every sweep and the trade lines
 *                     should not displace it: -4 % at 8M-16M pools -- and write-through stores otherwise; 1 = always
 *                     write-through (best while the market stays cache-resident between sweeps: route!); 2 = always
 *                     non-temporal: a caller that rotates over many markets, each of which fits the cache, says so: -2..-5 %
 *                     when the pool state really comes from HBM, +0..3 % when it does not),
 *                     "direct_small" (default 1: a context with one pool family and at most 2048 pools is swept by ONE block
 *                     that delivers {psi, acc} itself -- one kernel per evaluation instead of sweep + fold; 0: the general
 *                     two-launch geometry),
 *                     "univ3_heads" (default 1: multi-tick UniV3 walks decide their first four list ticks from a per-pool
 *                     head of rounded-down binary32 thresholds read with the pool's coalesced streams, and consult the
 *                     exact threshold array only for deeper walks or a price within 2^-23 of a threshold: same decisions,
 *                     same bits, 11 % fewer bytes; 0: always the exact array),
 *                     "lean_kernels" (default 1: a launch in the default configuration -- compact write-through trade
 *                     records, a fee table, prices staged as pairs, one bin copy per wavefront -- takes the form of its
 *                     kernel in which those are compile-time facts: same bits, fewer instructions per tile; 0: always the
 *                     general kernels; read-only "lean_launches": the sweep launches that took such a kernel)
 *   arithmetic        "fast_math" (default 1: where every operand lies in [2^-150, 2^150] -- pool constants checked at
 *                     upload, prices by the host (host-pointer calls, cfmm_route) and again by every block as it stages
 *                     them; the library then launches kernels in which divisions and square roots run the compiler's
 *                     own correctly-rounded instruction sequences WITHOUT their range scaffolding, and divisions by a
 *                     price or a fee reuse a reciprocal refined once per token / fee tier: same bits, ~half the
 *                     instructions; the log-space GeometricMean form -- within 1e-12 of the reference either way --
 *                     also evaluates its exponential with an own < 1 ulp polynomial instead of the device library's;
 *                     anything outside the window runs the full-range arithmetic -- device-pointer sweeps, whose prices
 *                     the library cannot see, decide per block inside the launch (cfmm_sweep_dev);
 *                     0: the compiler's sequences and the library's exp everywhere), "dev_prices_in_window" (default 0;
 *                     1 = the caller vouches that the prices it passes to cfmm_sweep_dev lie in [2^-150, 2^150] -- the
 *                     check the library makes itself on host-pointer calls -- and device-pointer sweeps launch the fast
 *                     kernels alone (fewer registers than the kernels that carry both arithmetics); every block still
 *                     checks the prices it stages, and a broken promise yields NaN in every entry of {psi, acc}: an
 *                     error, never a wrong number), "geomean_exact" (1 = GeometricMeanTwoCoin
 *                     with pow in the reference's operation order instead of the default log-space form; both are within
 *                     1e-12 of the reference), "alternate" (default 1: consecutive evaluations walk every lane's tiles in
 *                     alternating directions, so that a sweep starts on the pool data the previous one left in the XCD's
 *                     L2 -- two fused evaluations at the same v then agree to summation-order rounding, every second one
 *                     bit for bit.  cfmm_find_arb and the final sweep of cfmm_route always walk forwards: find_arb!(r, v)
 *                     is a function of v alone, and cfmm_route restarts the alternation, so a route is a function of its
 *                     arguments alone; 0: always forwards, every sweep bit-identical)
 *   host boundary     "zero_copy" (default 1: host-pointer calls read v through mapped pinned memory), "host_flag"
 *                     (default 1: such a call ends when {psi, acc} have arrived in pinned host memory as self-validating
 *                     8-byte granules, which the library polls, instead of on the stream's completion signal),
 *                     "time_kernels" (see cfmm_kernel_times), "multi_threads" (multi-device contexts)
 *   route!            "armed" (default 1: cfmm_route enqueues evaluation k+1 while evaluation k runs; its blocks wait on
 *                     the device -- bounded by "arm_timeout_ms", default 2000 -- until the host has written the next price
 *                     vector straight into device memory through the PCIe BAR, which takes the launch latency off the
 *                     critical path of every evaluation; needs a large-BAR system, otherwise -- or with CFMM_AMD_ARMED=0
 *                     in the environment -- the evaluations are launched when their prices are ready; identical results
 *                     either way; also on cfmm_set_peers contexts and on multi-device contexts whose shards sit on
 *                     distinct devices), "stop_in_noise" (default 0 = the stopping rules of L-BFGS-B 3.0, the
 *                     reference's solver; 1 = additionally end the run when a line-search trial point differs from the
 *                     current dual value by no more than the factr tolerance: fewer evaluations, v* up to a decade
 *                     further from the reference's).
 * Environment: HIP_FORCE_DEV_KERNARG is set to 1 when the library is loaded unless already set (kernel arguments in
 * device memory: -10 % per step); CFMM_AMD_PEER_TIMEOUT_S (see cfmm_set_peers). */
int cfmm_set_option(cfmm_ctx* ctx, const char* key, int64_t value);
int cfmm_get_option(const cfmm_ctx* ctx, const char* key, int64_t* value);

/* ---- pool upload (struct definitions + constructors, packed once) --------------------- */

/* m x ProductTwoCoin(R, gamma, idx) -- src/cfmms.jl:101-111 (+ checks of :76-90).
 * R[m][2] > 0, gamma[m] > 0, Ai[m][2] distinct and in [0, n_tokens). */
int cfmm_pools_add_product(cfmm_ctx* ctx, int64_t m, const double* R, const double* gamma,
                           const int32_t* Ai);

/* m x GeometricMeanTwoCoin(R, w, gamma, idx) -- src/cfmms.jl:152-165.  w[m][2] > 0. */
int cfmm_pools_add_geomean(cfmm_ctx* ctx, int64_t m, const double* R, const double* w,
                           const double* gamma, const int32_t* Ai);

/* m x UniV3(current_price, lower_ticks, liquidity, gamma, Ai) -- src/cfmms.jl:226-245,
 * ragged ticks in CSR form: pool i owns lower_ticks/liquidity[tick_off[i] .. tick_off[i+1]).
 * lower_ticks strictly descending and > 0 per pool, liquidity >= 0, and
 * current_price <= lower_ticks[first] (the reference would index tick 0 otherwise, :235,:316).
 * current_tick is derived here exactly as :235 does.  A stand-alone BoundedProduct pool
 * (src/cfmms.jl:272-289) is a UniV3 with two ticks whose second liquidity is 0. */
int cfmm_pools_add_univ3(cfmm_ctx* ctx, int64_t m, const double* current_price, const double* gamma,
                         const int32_t* Ai, const int64_t* tick_off, const double* lower_ticks,
                         const double* liquidity);

/* m x GeometricMean(R, w, gamma, Ai) with n_coins coins each -- src/cfmms.jl:57-64 (Product(R, gamma, Ai) = equal w:
 * the same level sets, hence the same trades).  The reference declares these N-coin CFMMs but gives them no find_arb!;
 * here the problem of its find_arb! docstring (src/cfmms.jl:21-33) is solved exactly per pool.
 * R[m][n_coins] > 0, w[m][n_coins] > 0 (normalised to sum to 1 per pool), Ai[m][n_coins] distinct and in
 * [0, n_tokens), 2 <= n_coins <= 8, and 0 < gamma <= 1: unlike the two-coin families, gamma > 1 is refused (a fee that pays
 * for round trips makes the N-coin problem unbounded).  Every call is its own segment (batches with different coin counts
 * go in separate calls) and its own launch: weighted segments are never fused with other families.  Trades are ragged:
 * see cfmm_get_trades.  n_tokens > 8192 (large-market mode) returns CFMM_ERR_UNSUPPORTED. */
int cfmm_pools_add_weighted(cfmm_ctx* ctx, int64_t m, int32_t n_coins, const double* R, const double* w,
                            const double* gamma, const int32_t* Ai);

/* m x Curve(R, gamma, Ai, alpha, beta) with n_coins coins each -- src/cfmms.jl:66-70.  Trading function
 *     phi(R) = alpha * sum_k R_k - beta / prod_k R_k,   alpha >= 0, beta > 0:
 * Curve's StableSwap invariant A n^n sum x + D = A D n^n + D^(n+1) / (n^n prod x) with D held fixed (a swap keeps D), i.e.
 * alpha = A n^n and beta = D^(n+1) / n^n (phi(R) = A D n^n - D on the pool's own reserves).  alpha = 0 trades exactly like
 * Product.  The reference declares Curve without a find_arb!; here the problem of its find_arb! docstring
 * (src/cfmms.jl:21-33) is solved per pool.  The fee is the reference's
 * input-side gamma, as for every family (not Curve's own output-side fee, which also grows D).
 * R[m][n_coins] > 0, Ai[m][n_coins] distinct and in [0, n_tokens), alpha[m] >= 0, beta[m] > 0, all finite,
 * 0 < gamma <= 1 (gamma > 1 is refused, as for weighted pools), 2 <= n_coins <= 8.  Every call is its own segment and its
 * own launch; trades are ragged (cfmm_get_trades); n_tokens > 8192 returns CFMM_ERR_UNSUPPORTED.
 * cfmm_update_reserves moves R and keeps alpha and beta (the pool's parameters). */
int cfmm_pools_add_curve(cfmm_ctx* ctx, int64_t m, int32_t n_coins, const double* R, const double* gamma,
                         const int32_t* Ai, const double* alpha, const double* beta);

/* m x SolidlyStableTwoCoin(R, gamma, idx): the "stable" pair of the Solidly family (Velodrome, Aerodrome and forks),
 *     phi(x, y) = x^3 y + x y^3   on decimal-normalised balances.
 * The reference has no such pool; solved here is the problem of its find_arb! docstring (src/cfmms.jl:21-33), which has a
 * closed form for this phi: one cbrt, two square roots and five divisions per trading pool.  The
 * fee is the reference's input-side gamma, as for every family.
 * Array shapes and checks of cfmm_pools_add_product, plus: gamma <= 1 (gamma > 1 is refused, as for the N-coin families:
 * the closed form assumes that at most one direction trades) and every reserve within [2^-150, 2^150] (the cube of
 * R2/R1 must stay finite).  A two-coin kind: its trades live in the common [m][2] buffers (cfmm_get_trades,
 * cfmm_trades_dev), large-market mode (n_tokens > 8192) works, cfmm_update_reserves applies R <- (R + gamma Delta) - Lambda.
 * Every call is its own segment and its own launch (never fused with other families); one arithmetic (the compiler's
 * full-range division, square root and cbrt; option "fast_math" does not apply). */
int cfmm_pools_add_solidly(cfmm_ctx* ctx, int64_t m, const double* R, const double* gamma, const int32_t* Ai);

int cfmm_pools_clear(cfmm_ctx* ctx);
int64_t cfmm_pools_count(const cfmm_ctx* ctx); /* length(r.cfmms) */
int32_t cfmm_n_tokens(const cfmm_ctx* ctx);    /* length(r.v) */

/* ---- the hot path --------------------------------------------------------------------- */

/* find_arb!(r::Router, v) -- src/router.jl:38-42, dispatching to src/cfmms.jl:130-140,
 * :185-196, :339-395 per segment.  Materialising sweep: writes every pool's Delta/Lambda
 * to device memory AND reduces psi = sum_i A_i(Lambda_i - Delta_i) and the dual scalar
 * acc = sum_i (Lambda_i - Delta_i)'v[A_i] in the same pass.  v: n_tokens host doubles. */
int cfmm_find_arb(cfmm_ctx* ctx, const double* v);

/* The evaluation route!'s closures fn / g! need (src/router.jl:73-86, :89-102) without the
 * O(m) trade write-back: psi_out[n_tokens] = pool part of G (== netflows at v),
 * *acc_out = pool part of fn.  Either output pointer may be NULL. */
int cfmm_eval(cfmm_ctx* ctx, const double* v, double* psi_out, double* acc_out);

/* r.Δs / r.Λs after find_arb! -- src/router.jl:7-8,40, flattened: cfmm_trades_len doubles each, segment order, each
 * pool's coins in its Ai order (2 per two-coin pool, n_coins per weighted or Curve pool).  Without weighted or Curve pools that is exactly
 * [m_total][2].  Requires a preceding cfmm_find_arb (cfmm_eval does not produce trades). */
int cfmm_get_trades(cfmm_ctx* ctx, double* Delta, double* Lambda);
/* Length of each array cfmm_get_trades writes: the sum over pools of their coin counts. */
int64_t cfmm_trades_len(const cfmm_ctx* ctx);
/* Same, one segment: rows [first, first+count) of segment `seg` (count x n_coins doubles for a weighted segment). */
int cfmm_get_trades_range(cfmm_ctx* ctx, int32_t seg, int64_t first, int64_t count, double* Delta,
                          double* Lambda);

/* The rows of segment `seg` that trade in the latest materialising sweep and are worth at least min_value,
 * in pool order: the short list a router that follows a chain executes, compacted ON THE DEVICE (three small launches: flag +
 * count, scan, emit; no block waits for another) instead of downloading and scanning every pool's rows.
 *   Rule       pool i trades iff some entry of its Delta or Lambda compares != 0.0 (-0.0 does not count, NaN does).
 *   Value      value_i = sum_k (Lambda_ik - Delta_ik) * v[A_ik], the pool's term of the dual acc: summed in the pool's coin
 *              order from +0.0, every subtraction, product and addition rounded on its own (no FMA), so that the host can
 *              reproduce it bit for bit.
 *   Selection  a row is selected iff it trades and !(value_i < min_value): a NaN value is never hidden, and
 *              min_value = -INFINITY selects every trading pool.
 *   v          n_tokens host doubles, the prices the trades are valued at; not range-checked (NaN propagates into value).
 *              NULL: the prices of the latest materialising host-pointer sweep (cfmm_find_arb, cfmm_route).  After a
 *              materialising cfmm_sweep_dev the library has not seen the prices: NULL is then CFMM_ERR_STATE, an explicit v works.
 *   Outputs    *count = the number of selected rows, whatever `capacity` is.  The first min(count, capacity) selected rows, in
 *              ascending pool order, go to idx[] (rows within the segment, as in cfmm_get_trades_range), Delta[][n_coins] and
 *              Lambda[][n_coins] (the reference's rows, bit-identical to cfmm_get_trades_range for those rows; n_coins = 2, or
 *              the coin count of a weighted / Curve segment) and value[].  idx, Delta, Lambda and value may each be NULL;
 *              capacity == 0 counts only; exactly min(count, capacity) rows are written, the rest of the arrays stays untouched.
 *              capacity < 0, count == NULL or a bad seg: CFMM_ERR_INVALID_ARG.
 *   State      needs materialised trades (else CFMM_ERR_STATE, "no materialised trades", as cfmm_get_trades); consumes nothing and
 *              invalidates nothing: cfmm_get_trades, cfmm_update_reserves and cfmm_trades_dev behave afterwards as if it had not
 *              been called.  Synchronous, on the context's stream, behind the sweep.
 * Works on every kind, both trade layouts (option "compact_trades"), large-market mode and multi-device contexts (the shards
 * that hold rows of `seg` are asked in device order, which is pool order; counts are summed).  On a context sharded with
 * cfmm_set_peers or RCCL the call is LOCAL to the rank's own pools and is not collective: no other rank needs to make it.
 * Read-only options: "select_block_pools" and "select_scan_chunk" (the launch geometry: pools per block, block counts per scan
 * step), and, under option "time_kernels", "select_flag_ns" / "select_scan_ns" / "select_emit_ns": the kernel spans of the
 * latest call. */
int cfmm_select_trades(cfmm_ctx* ctx, int32_t seg, const double* v, double min_value, int64_t capacity,
                       int64_t* count, int64_t* idx, double* Delta, double* Lambda, double* value);

/* update_reserves!(r) -- src/router.jl:127-132.  The reference's router method calls a per-pool
 * update_reserves!(c, Δ, Λ, v) that is defined nowhere (its own test is disabled, test/arb.jl:30-39);
 * implemented here is the update the routing problem prescribes (find_arb! docstring,
 * src/cfmms.jl:26-31: the pool ends at R + γΔ − Λ), applied IN PLACE ON THE DEVICE from the trades of
 * the latest materialising sweep (cfmm_find_arb, cfmm_route; consumed by this call):
 *   ProductTwoCoin / GeometricMeanTwoCoin:  R <- (R + γΔ) − Λ            (one kernel, no host traffic)
 *   Solidly stable pairs (CFMM_KIND_SOLIDLY): R <- (R + γΔ) − Λ           (the same kernel)
 *   weighted (CFMM_KIND_WEIGHTED):          R <- (R + γΔ) − Λ per coin    (one kernel, no host traffic)
 *   Curve (CFMM_KIND_CURVE):                R <- (R + γΔ) − Λ per coin    (one kernel; α, β unchanged)
 *   UniV3 / BoundedProduct: the state is the price.  A pool that traded moves to the internal price
 *     P = p/γ (price falling, src/cfmms.jl:361) or γ·p (price rising, :381), p = v₁/v₂, clamped to the
 *     first tick's upper price; its tick constants are re-derived as at upload (:294-313).  That is
 *     exactly the pool R + γΔ − Λ tick by tick (tested), and needs the prices of the trades: the
 *     materialising sweep must have been a host-pointer call.
 * Afterwards a sweep at the same prices finds no arbitrage in any pool. */
int cfmm_update_reserves(cfmm_ctx* ctx);
/* Current reserves R[m][2] of a two-coin segment (R[m][n_coins] of a weighted or Curve one) / current prices [m] of a UniV3 segment. */
int cfmm_get_reserves(cfmm_ctx* ctx, int32_t seg, double* R);
int cfmm_get_prices(cfmm_ctx* ctx, int32_t seg, double* current_price);

/* Sparse pool-state updates: the reference's `cfmm.R .= ...` (or a new `current_price`) on a few pools of a router,
 * followed by another route! -- what a router that follows a chain does every block.  The new state of `count` pools of
 * ONE segment replaces the old one on the device; everything else of the market (tokens, fees, weights, tick ladders,
 * the launch plan, fee tables, packed records, large-market incidence lists) stays as uploaded, and nothing is re-uploaded.
 *   seg   segment index as in cfmm_segment_info / cfmm_get_reserves; idx[0..count) rows within it, in any order.  A row
 *         named more than once takes the value of its LAST occurrence (decided on the host).  count == 0: a no-op.
 *   cfmm_pools_set_reserves  ProductTwoCoin, GeometricMeanTwoCoin, Solidly and weighted segments: R[count][n_coins]
 *   cfmm_pools_set_curve     Curve segments: R[count][n_coins] with the pools' alpha[count], beta[count] (A ramps; D, hence
 *                            beta, moves with liquidity and fees)
 *   cfmm_pools_set_prices    UniV3 segments: current_price[count]; ticks and liquidity stay (a mint / burn:
 *                            cfmm_pools_set_ticks)
 *   cfmm_pools_set_ticks     UniV3 segments: a mint or a burn.  The rows' NEW tick ladders in CSR form over the count rows
 *                            (tick_off[count + 1], tick_off[0] == 0; lower_ticks and liquidity [tick_off[count]], in the
 *                            parametrisation of cfmm_pools_add_univ3) and a current price per row (the old one for a pure
 *                            mint / burn).  A ladder may grow, shrink or move; the segment's tick total 2·(T + 2m) <=
 *                            0x3fffffff is checked on the new total (CFMM_ERR_UNSUPPORTED)
 * The entry that does not fit the segment's kind returns CFMM_ERR_INVALID_ARG and names the one that does; so does a seg or
 * an idx out of range.
 * Checks: those of the matching cfmm_pools_add_*, in its order and with its error texts (the pool number is the row), on
 * the values given: reserves finite and > 0; Solidly reserves within [2^-150, 2^150]; Curve alpha >= 0, beta > 0 and, with
 * alpha > 0, log(P0/R_k) within the solve's range; a price finite, > 0 and not above the pool's first tick; a new ladder
 * of at least one tick, tick prices finite, > 0 and strictly descending, liquidity finite and >= 0.  ALL rows are
 * checked before anything changes: a refused call leaves the context exactly as it was, on the host and on the device.
 * Prepared constants (GeometricMean {Q1, Q2}, weighted log(R / w), Curve log R and {alpha, log beta}, every UniV3 record:
 * current-tick constants, walk lists with their running sums, drain thresholds, heads) are computed ON THE HOST with the
 * upload's own code, so an updated context equals, bit for bit on every output, a context freshly uploaded with the new
 * state (cfmm_update_reserves, whose logarithms run on the device, promises no such thing).
 * A value outside [2^-150, 2^150] sends a Product / GeometricMean / UniV3 segment to the full-range arithmetic (same bits),
 * as cfmm_update_reserves does; an update never sends it back: only cfmm_pools_clear + a re-add does.
 * The update is enqueued on the context's stream behind earlier sweeps; the trades and outputs of earlier sweeps are
 * invalidated as by cfmm_update_reserves (cfmm_get_trades then fails with "no materialised trades" until the next
 * cfmm_find_arb / cfmm_route).  The walk lists of a moved UniV3 pool are appended to the segment's record arrays, whose
 * spare room is grown geometrically and compacted when it runs out: one kernel on the stream (compact_walks) copies the
 * records in use into fresh arrays, no record crosses PCIe (counted by the read-only option "pool_update_regrows"; with
 * "time_kernels" the kernel's span is the read-only option "compact_walks_ns").  An upload allocates no spare room, so the
 * first update of a UniV3 segment compacts.  cfmm_pools_set_ticks keeps the launch plan unless the segment's mean ticks
 * per pool crosses 2 or its first walk list appears; then the plan is rebuilt at the next sweep, as after an upload.
 * Multi-device contexts: the rows are split over the shards; every shard checks its rows before any shard changes.
 * Limits: not for adding or removing pools, nor for tokens, fees or weights (cfmm_pools_clear + re-add). */
int cfmm_pools_set_reserves(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const double* R);
int cfmm_pools_set_curve(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const double* R,
                         const double* alpha, const double* beta);
int cfmm_pools_set_prices(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const double* current_price);
int cfmm_pools_set_ticks(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const double* current_price,
                         const int64_t* tick_off, const double* lower_ticks, const double* liquidity);

/* Exact-input swap quotes: "if I tender amount_in of coin_in to this pool as it stands on the device now, how much of
 * coin_out comes out?"  Generalises forward_trade(Δ, cfmm::UniV3), src/cfmms.jl:398-449 -- the reference's only quote -- to
 * every kind: amount_out is the largest out >= 0 with φ(R + γ·a·e_in − out·e_out) = φ(R), the constraint of src/cfmms.jl:26-31
 * (fee on the input) met with equality.  Closed forms, one lane per query, no iteration (UniV3: a search on the running sums
 * of the walk records plus one closed form).  amount_in == 0 gives exactly +0.0.
 *   seg        as in cfmm_segment_info.
 *   idx        [count] rows within the segment, in any order, repeats allowed (a ladder of sizes through one pool is
 *              `count` queries on the same row).  NULL: rows 0 .. count-1.
 *   coin_in,   [count] positions in the pool's own coin order (0-based, < n_coins), NOT token numbers.  coin_out == NULL is
 *   coin_out   allowed on two-coin and UniV3 segments and means 1 - coin_in; on weighted / Curve segments NULL is
 *              CFMM_ERR_INVALID_ARG.
 *   amount_in  [count], finite and >= 0.        amount_out  [count].
 * cfmm_quote (host pointers) checks everything before anything is enqueued -- seg, count >= 0, every row in range, coins in
 * range and distinct, amounts finite and >= 0; a failure is CFMM_ERR_INVALID_ARG, names the query in cfmm_last_error and
 * leaves amount_out untouched.  Synchronous on the context's stream, behind earlier sweeps and updates.  count == 0: a no-op.
 * UniV3: a tendered amount beyond all liquidity of the direction returns the whole of it ("exhausted all liquidity", :432); the
 * unused input is not reported, as in the reference.
 * Read-only: consumes nothing and invalidates nothing -- cfmm_get_trades*, cfmm_select_trades, cfmm_netflows,
 * cfmm_update_reserves, a pre-armed cfmm_route and the next sweep behave as if it had not been called; needs no sweep to
 * have run.  Works on every kind, in large-market mode and on multi-device contexts (the queries are split over the shards
 * that hold their rows; the answers return in query order).  On a context sharded with cfmm_set_peers or RCCL the call is
 * LOCAL to the rank's own pools and is not collective.  Device memory of the call is proportional to count, never to the pools.
 * Read-only option under "time_kernels": "quote_ns", the span of the latest call's kernel (a multi-device context: the longest
 * among the shards that call touched; after cfmm_quote_dev, reading it waits for the kernel). */
int cfmm_quote(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
               const int32_t* coin_out, const double* amount_in, double* amount_out);
/* The same on device arrays (src/cfmms.jl:398-449 generalised, as cfmm_quote): asynchronous on the context's stream; checks
 * only seg and count (and that coin_out is given where it must be).  The library cannot validate device memory: an
 * out-of-range row or coin, equal coins, or a negative or non-finite amount yields NaN for THAT query and correct answers
 * for the rest; indices are clamped before any read, so the call never reads out of bounds.  Single-device contexts only. */
int cfmm_quote_dev(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                   const int32_t* d_coin_out, const double* d_amount_in, double* d_amount_out);

/* Exact-output swap quotes, the inverse of cfmm_quote: "I need exactly amount_out of coin_out from this pool as it stands on
 * the device now; how much of coin_in must I tender?"  (The reference has no such function; the constraint is the one of
 * src/cfmms.jl:26-31, fee on the input.)  amount_in is the smallest a >= 0 with φ(R + γ·a·e_in − amount_out·e_out) = φ(R).
 * Closed forms, one lane per query, no iteration (UniV3: a search on the running sums ΣR_out of the walk records plus one
 * closed form).  amount_out == 0 gives exactly +0.0.  Where no finite input yields amount_out the answer is
 * +inf, NOT an error: amount_out >= the pool's reserve of coin_out on the reserve kinds; on UniV3 an amount beyond the
 * direction's total liquidity, or equal to a total that is only approached (the direction's last tick reaches down to price
 * 0).  On UniV3 an amount_out equal to the total of a direction that a finite input exhausts gives that input, so
 * cfmm_quote_out(cfmm_quote(a)) is the input the pool actually consumed when `a` exhausts the ladder.
 * seg, idx, coin_in, coin_out, count == 0, the checks (amount_out finite and >= 0; a failure is CFMM_ERR_INVALID_ARG, names the
 * query with the prefix "cfmm_quote_out:" and leaves amount_in untouched), the synchronisation, the read-only guarantees, large-
 * market mode, multi-device and sharded contexts: exactly as cfmm_quote.  "quote_ns" reports the latest call of either
 * direction.  The direction rule on UniV3 is cfmm_quote's: coin 0 in walks the price-falling list. */
int cfmm_quote_out(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                   const int32_t* coin_out, const double* amount_out, double* amount_in);
/* The same on device arrays, as cfmm_quote_dev is to cfmm_quote: asynchronous on the context's stream; checks only seg and
 * count (and that coin_out is given where it must be); an out-of-range row or coin, equal coins, or a negative or non-finite
 * amount_out yields NaN for THAT query; indices are clamped before any read.  Single-device contexts only. */
int cfmm_quote_out_dev(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* d_idx, const int32_t* d_coin_in,
                       const int32_t* d_coin_out, const double* d_amount_out, double* d_amount_in);

/* Multi-hop path quotes: an amount carried through a PATH of pools that may lie in different segments (and therefore be of
 * different kinds), one launch for all paths.  (The reference has no such function; each hop is the constraint of
 * src/cfmms.jl:26-31 as in cfmm_quote / cfmm_quote_out.)  A path has 1 .. CFMM_MAX_PATH_HOPS hops; a hop is
 * (segment, row, coin_in, coin_out), coins being positions in the pool's own coin order.
 *   cfmm_quote_path      exact input:  x_0 = amount_in[p], x_{k+1} = quote(hop k, x_k); amount_out[p] = x_H.
 *   cfmm_quote_path_out  exact output: y_H = amount_out[p], y_k = quote_out(hop k, y_{k+1}), walked from the last hop to the
 *                        first; amount_in[p] = y_0.  Once a hop answers +inf (that pool cannot give that much) every earlier
 *                        hop and the answer are +inf and no further form is evaluated: an answer, not an error.  NaN likewise.
 * The per-hop arithmetic is cfmm_quote's / cfmm_quote_out's own: the result and every intermediate amount equal, bit for bit,
 * what chaining those calls hop by hop gives (UniV3: an exhausted ladder returns the direction's whole output, same direction rule).
 * EVERY HOP IS QUOTED AGAINST THE POOL AS IT STANDS: no state advances between hops.  A path that visits a pool twice has its
 * second visit quoted as if the first had not happened; the call does not refuse such a path.  Amounts pass from hop to hop
 * whatever the tokens are: token continuity is the caller's business.
 *   n_hops        [count], each 1 .. max_hops.       max_hops  1 .. CFMM_MAX_PATH_HOPS: the rows of the hop arrays.
 *   hop_seg, hop_row, hop_coin_in, hop_coin_out   [max_hops][count], HOP-MAJOR: hop k of path p at k*count + p.  Slots at
 *                 k >= n_hops[p] are ignored.  hop_coin_out is always required (there is no "other coin" default here).
 *   hop_out       NULL, or [max_hops][count]: hop_out[k*count+p] = the amount leaving hop k (so the entry of a path's last hop
 *                 equals amount_out[p]).   hop_in: hop_in[k*count+p] = the amount to tender to hop k (hop_in[p] == amount_in[p]).
 *                 Unused slots are written as NaN.
 * The host-pointer entries check everything before anything is enqueued: count >= 0, max_hops, every n_hops, every used
 * hop's segment, row and coins in range for that segment, coins distinct, the given amount finite and >= 0.  A failure is
 * CFMM_ERR_INVALID_ARG, names the path and the hop ("cfmm_quote_path: path 12, hop 3: row ...") and leaves the outputs
 * untouched.  Synchronous on the context's stream; read-only exactly as cfmm_quote; count == 0 is a no-op; large-market mode
 * needs nothing special; on a context sharded with cfmm_set_peers or RCCL the call is local to the rank.  On a multi-device
 * context a path's hops may sit on different shards: the paths are walked hop level by hop level through cfmm_quote /
 * cfmm_quote_out (one call per level and segment with an active path), the +inf / NaN rule applied on the host -- the same bits.
 * "quote_ns" reports the latest call of any quote entry (a multi-device context: the longest span among the calls this entry made). */
#define CFMM_MAX_PATH_HOPS 8
int cfmm_quote_path(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                    const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_in,
                    double* amount_out, double* hop_out);
int cfmm_quote_path_out(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                        const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_out,
                        double* amount_in, double* hop_in);
/* The same on device arrays: asynchronous on the context's stream; checks only the scalars and null pointers (d_hop_out /
 * d_hop_in may be NULL).  The library cannot validate device memory: an n_hops outside 1 .. max_hops makes that path NaN with
 * no hop evaluated; a hop with an out-of-range segment, row or coin, equal coins, or a negative or non-finite amount is clamped
 * before any read and yields NaN, which then passes through the path's remaining hops.  Nothing is read out of bounds and
 * neighbouring paths are unaffected.  Single-device contexts only. */
int cfmm_quote_path_dev(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                        const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                        const double* d_amount_in, double* d_amount_out, double* d_hop_out);
int cfmm_quote_path_out_dev(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* d_n_hops, const int32_t* d_hop_seg,
                            const int64_t* d_hop_row, const int32_t* d_hop_coin_in, const int32_t* d_hop_coin_out,
                            const double* d_amount_out, double* d_amount_in, double* d_hop_in);

/* Exact-input swaps that MOVE the pools: "tender amount_in of coin_in to this pool, take what comes out, and carry on from
 * the market that leaves behind" -- the other half of cfmm_quote.  (The reference has no such function; the move is the update
 * of src/cfmms.jl:26-31 that cfmm_update_reserves applies to the router's own trades.)  The argument list is cfmm_quote's:
 * seg, idx (NULL: rows 0 .. count-1), coin_in, coin_out (NULL allowed on two-coin and UniV3 segments, refused on weighted /
 * Curve), amount_in finite and >= 0.  All of cfmm_quote's checks run before anything is enqueued: a failure is
 * CFMM_ERR_INVALID_ARG, names the query in cfmm_last_error with the prefix "cfmm_swap:", and leaves amount_out AND the
 * pools untouched.
 * The swaps are applied IN QUERY ORDER.  For q = 0, 1, ...: amount_out[q] is exactly, bit for bit, what cfmm_quote answers
 * for that query on the pool as it stands after swaps 0 .. q-1; the pool then moves to R + γΔ − Λ with Δ = amount_in·e_in,
 * Λ = amount_out·e_out.  A row named k times is swapped k times, each from the state the previous one left.
 *   Reserve kinds (Product, GeometricMean, Solidly, weighted, Curve): R_in <- R_in + γ·a, R_out <- R_out − out, each operation
 *     rounded on its own; the other coins are untouched.  The prepared constants are refreshed on the device with
 *     cfmm_update_reserves' expressions: GeometricMean {Q1, Q2}; weighted q = log(R/w) and Curve q = log R for the two coins
 *     that moved (Curve's α and β stay).  amount_in == 0 leaves every bit of the pool.  A reserve leaving the window of the
 *     fast arithmetic sends the segment to full-range arithmetic for good, as cfmm_update_reserves does.
 *   UniV3: the state is the price.  The new price is computed on the device from the record the swap lands in -- inside the
 *     current tick when it holds liquidity and γa < its δmax, else record e of the direction's walk list with
 *     d_t = γa − Σδmax_e clamped to [0, δmax_e]; with s' = s_in + d_t, P = k/(s'·s') for coin 0 in (price falling) and
 *     P = (s'·s')/k for coin 1 in (price rising).  A swap that exhausts the direction answers cfmm_quote's whole output and
 *     rests at the far edge of the direction's last non-empty tick (that tick at d_t = δmax).  amount_in == 0, or a direction
 *     without any liquidity, leaves the price where it is.  The host reads the new prices back (8 bytes per swap), clamps
 *     each to the pool's first tick's upper price as cfmm_update_reserves does, and moves the pools through
 *     cfmm_pools_set_prices' own apply path: afterwards the context equals, bit for bit on every output, a context freshly
 *     uploaded at cfmm_get_prices' values.
 * A swap that would leave a pool cfmm_pools_set_* refuses -- a new reserve that is not finite and > 0 (a huge amount_in on a
 * Product pool, where x/(R_in + x) rounds to 1), a Solidly reserve outside [2^-150, 2^150], a Curve log(P0/R_k) outside the
 * solve's range, a UniV3 price that is not finite and > 0 -- is NOT APPLIED: that pool stays exactly as it was, its amount_out
 * is NaN, later swaps of the same row proceed from the unchanged state, and the call still returns CFMM_OK.  The read-only
 * option "swap_refused" is the number of such swaps in the latest call.
 * cfmm_swap is a state change, not a query: it invalidates the trades and outputs of earlier sweeps exactly as
 * cfmm_pools_set_reserves does (cfmm_get_trades* then fail with "no materialised trades", a pre-armed cfmm_route is
 * cancelled).  Synchronous on the context's stream, behind earlier sweeps and updates.  count == 0 is a no-op that
 * invalidates nothing.  Needs no sweep to have run; large-market mode needs nothing special; on a context sharded with
 * cfmm_set_peers or RCCL the call is local to the rank.  On a multi-device context the swaps go to the shards that hold
 * their rows (a row lives on one shard, so per-row order is kept), the answers return in query order, and every check runs
 * before any shard changes.  Device memory of the call is proportional to count, never to the pools.
 * Repeated rows are ordered on the host: swap q runs in launch number (earlier queries on the same row), each launch holds
 * distinct rows only.  A batch of distinct rows is one launch; UniV3 re-prepares the moved pools on the host after each launch.
 * There is NO cfmm_swap_dev: the order of repeated rows is decided on the host, and an unchecked device array cannot promise it.
 * Read-only option under "time_kernels": "swap_ns", the sum of the kernel spans of the latest call (a multi-device context:
 * the longest among the shards that call touched). */
int cfmm_swap(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
              const int32_t* coin_out, const double* amount_in, double* amount_out);

/* Exact-output swaps that MOVE the pools: "I must receive exactly amount_out of coin_out from this pool; take what that
 * costs, unless it costs more than max_amount_in" -- the other half of cfmm_quote_out, and cfmm_swap's mirror image.  The
 * arguments are cfmm_quote_out's plus max_amount_in, NULL (no limit) or [count], each finite and >= 0, and status, NULL or
 * [count].  All of cfmm_quote_out's checks and the limit check run before anything is enqueued: a failure is
 * CFMM_ERR_INVALID_ARG, names the query in cfmm_last_error with the prefix "cfmm_swap_out:", and leaves the outputs AND the
 * pools untouched.
 * The swaps are applied IN QUERY ORDER.  For q = 0, 1, ...: amount_in[q] is exactly, bit for bit, what cfmm_quote_out answers
 * for that query on the pool as swaps 0 .. q-1 left it (the kernel runs cfmm_quote_out's own function).  The swap then
 * delivers exactly the amount asked for -- not cfmm_quote(amount_in), which differs from it by rounding:
 *   Reserve kinds: R_in <- R_in + γ·amount_in, R_out <- R_out − amount_out, each operation rounded on its own; prepared
 *     constants and the fast-arithmetic window flag exactly as in cfmm_swap.
 *   UniV3: the state is the price, and the price is determined by the input: the pool rests at the price cfmm_swap of
 *     amount_in comes to rest at (the same function on the device, the same clamp and re-preparation on the host), so a
 *     UniV3 pool is left, bit for bit, where cfmm_swap of amount_in leaves it.  cfmm_quote_out finds its record on the running
 *     sums of the ticks' outputs and the landing price finds its own on the running sums of their inputs; when amount_out
 *     equals a running output sum at a tick boundary the two may name neighbouring records, which is harmless: the price is
 *     continuous across the boundary.
 * amount_out == 0 answers +0.0 and leaves every bit of the pool (status CFMM_SWAP_APPLIED).
 * A swap is NOT APPLIED in three cases, tested in this order; in each the pool keeps every bit, later swaps of that row
 * proceed from the unchanged state, and the call still returns CFMM_OK.  status[q]:
 *   CFMM_SWAP_APPLIED       applied                  amount_in[q] the answer
 *   CFMM_SWAP_UNOBTAINABLE  cfmm_quote_out answers +inf (the pool cannot give that much)   amount_in[q] +inf
 *   CFMM_SWAP_REFUSED       the new state is one cfmm_pools_set_* refuses -- cfmm_swap's conditions, unchanged; on UniV3 a
 *                           landing price that is not finite and > 0                       amount_in[q] NaN
 *   CFMM_SWAP_OVER_LIMIT    !(amount_in[q] <= max_amount_in[q])                            amount_in[q] the quote it would have cost
 * "swap_refused" is the number of swaps of the latest call whose status is not CFMM_SWAP_APPLIED.
 * Everything else is cfmm_swap's: the invalidation of earlier trades and outputs, count == 0 as a no-op, synchronous on the
 * context's stream, repeated rows ordered on the host in launches of distinct rows (one launch per wave, UniV3 pools moved
 * on the host between them), no _dev form, "swap_ns" and "swap_launches", device memory proportional to count; on a
 * multi-device context the swaps go to the shards that hold their rows, every check runs before any shard changes, and
 * amount_in and status return in query order. */
#define CFMM_SWAP_APPLIED 0      /* == CFMM_PATH_APPLIED */
#define CFMM_SWAP_OVER_LIMIT 1   /* == CFMM_PATH_BELOW_LIMIT's value: "the limit was not met" */
#define CFMM_SWAP_REFUSED 2      /* == CFMM_PATH_REFUSED */
#define CFMM_SWAP_UNOBTAINABLE 3 /* the pool cannot give that much: cfmm_quote_out answers +inf */
int cfmm_swap_out(cfmm_ctx* ctx, int32_t seg, int64_t count, const int64_t* idx, const int32_t* coin_in,
                  const int32_t* coin_out, const double* amount_out, const double* max_amount_in, double* amount_in,
                  int32_t* status);

/* Exact-input swap PATHS that MOVE their pools, each path all or nothing: what a transaction does on a chain -- it runs in
 * order, reverts whole, and carries a slippage limit.  The path arguments are exactly cfmm_quote_path's (hop-major
 * [max_hops][count], 1 .. CFMM_MAX_PATH_HOPS hops, slots at k >= n_hops[p] ignored); min_amount_out is NULL (no limit) or
 * [count], each finite and >= 0; hop_out and status may be NULL.
 * The paths are applied IN QUERY ORDER: path p sees the market as the APPLIED paths among 0 .. p-1 left it.  For an applied
 * path, amount_out[p] and every hop_out[k*count+p] are, bit for bit, what cfmm_quote_path answers for that path on that
 * market, and each hop's pool is then left exactly where cfmm_swap of (that hop, the amount entering it) leaves it: the
 * reserve kinds at R_in + γ·a, R_out − out with the prepared constants refreshed and the fast-arithmetic window flag kept per
 * segment; UniV3 at the price the hop comes to rest at, clamped on the host and moved through cfmm_pools_set_prices' own
 * apply path.  A hop entered with amount 0 leaves every bit of its pool.  The call therefore equals chaining cfmm_swap hop by
 * hop, path by path, in answers and in final state.
 * A POOL MAY APPEAR ONLY ONCE IN A PATH: a path that names one (segment, row) twice is refused.  With distinct pools the hops
 * of one path do not see each other's moves, so the whole path is quoted against the market as it stands and applied
 * afterwards -- which is what makes all-or-nothing possible without unwinding anything.  (cfmm_quote_path, which moves
 * nothing, does not refuse such a path.)
 * ALL OR NOTHING.  A path is applied only if (a) no hop would leave a pool that cfmm_pools_set_* refuses -- cfmm_swap's
 * refusal conditions, unchanged -- and (b) amount_out[p] >= min_amount_out[p] where a limit is given.  Otherwise none of its
 * pools changes a bit and later paths proceed from the unchanged market.  status[p]:
 *   CFMM_PATH_APPLIED      applied              amount_out[p] the answer, hop_out the hop amounts
 *   CFMM_PATH_BELOW_LIMIT  below the limit      amount_out[p] the quote it would have given, hop_out the hop amounts
 *   CFMM_PATH_REFUSED      a hop was refused    amount_out[p] NaN, hop_out the amounts before the refusing hop, NaN from it on
 * The call returns CFMM_OK in all three cases; afterwards "swap_refused" is the number of paths whose status is not
 * CFMM_PATH_APPLIED.  Unused hop_out slots are written as NaN.
 * Everything is checked before anything is enqueued: cfmm_quote_path's checks, the repeated pool ("cfmm_swap_path: path 3,
 * hops 0 and 2: ...") and the limits.  A failure is CFMM_ERR_INVALID_ARG, names the path and the hop(s), and leaves the
 * outputs AND the pools untouched.
 * A state change with cfmm_swap's protocol: the trades and outputs of earlier sweeps are invalidated, a pre-armed cfmm_route
 * is cancelled; synchronous on the context's stream; count == 0 is a no-op that invalidates nothing; on a context sharded
 * with cfmm_set_peers or RCCL the call is local to the rank.  Device memory of the call is proportional to count x max_hops,
 * never to the pools.  A MULTI-DEVICE CONTEXT answers CFMM_ERR_UNSUPPORTED before anything moves: a path's hops may sit on
 * different shards, and all-or-nothing across devices is a change of its own.
 * Paths that share pools are ordered on the host: a path runs in the first launch in which all its pools are free, a pool
 * being taken, for that launch, by every earlier path that names it -- applied or not, the host cannot know in advance.  Each
 * launch holds pool-disjoint paths only; a batch of pool-disjoint paths is one launch; the host waits between launches only
 * behind one with a UniV3 hop, whose pools it re-prepares.  There is NO cfmm_swap_path_dev, for cfmm_swap's reason: the
 * order is decided on the host.  The exact-output form, cfmm_swap_path_out, is declared in
 * cfmm_amd_path_out.h.
 * Read-only options: "swap_launches", the number of launches (waves) of the latest cfmm_swap* call; under
 * "time_kernels", "swap_ns", the sum of their kernel spans. */
#define CFMM_PATH_APPLIED 0
#define CFMM_PATH_BELOW_LIMIT 1
#define CFMM_PATH_REFUSED 2
int cfmm_swap_path(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* n_hops, const int32_t* hop_seg,
                   const int64_t* hop_row, const int32_t* hop_coin_in, const int32_t* hop_coin_out, const double* amount_in,
                   const double* min_amount_out, double* amount_out, double* hop_out, int32_t* status);

/* The best swap path between two tokens, FOUND on the device: "I have amount_in of token_in and want token_out -- through
 * which pools, and how much do I get?"  (The reference has no such function: route! with a Swap objective, src/objectives.jl:133-150,
 * answers with the optimal SPLIT over the whole market as per-pool trades; this entry answers with ONE executable path, the
 * thing cfmm_quote_path prices and cfmm_swap_path executes.)  Per query q: token_in[q], token_out[q] (0-based, < n_tokens),
 * amount_in[q] finite and >= 0, and at most max_hops (1 .. CFMM_MAX_PATH_HOPS) hops.
 * THE CONTRACT IS THE LAYERED SEARCH, on the market as it stands on the device:
 *   best[0][token_in] = amount_in; everything else is unreached.
 *   best[h][t], h = 1 .. max_hops: the maximum of quote(pool, ci -> co, best[h-1][tok(ci)]) over every pool of every segment
 *   and every ordered pair of its coins (ci, co) with tok(co) == t whose source best[h-1][tok(ci)] is reached.  A quote that is
 *   NaN, not finite or <= 0 enters nothing.
 *   amount_out = the maximum over h >= 1 of best[h][token_out]; the path has the FEWEST hops h* that attain it bit for bit, and
 *   is walked back from (h*, token_out): at each layer the hop is the SMALLEST (segment, row, coin_in, coin_out), in
 *   lexicographic order, among the edges that attain best[h][t] bit for bit.
 * So the answer is a pure function of the market and the query -- not of launch geometry, the order atomics arrive in or how
 * queries are batched.  The quotes are cfmm_quote's own, and EVERY HOP IS QUOTED AGAINST THE POOL AS IT STANDS, cfmm_quote_path's
 * rule: cfmm_quote_path on the returned arrays answers amount_out bit for bit, and every intermediate amount with it.
 * What is found is a WALK, not a simple path: it may pass a token twice and may visit a pool twice (quoted twice from the same
 * reserves); a search constrained to simple paths is not offered.  Where every pool's quote is non-decreasing in its input --
 * it is mathematically; rounding can break it by ulps -- the layered maximum is the maximum over all walks of at most
 * max_hops hops; the contract is the layered one, not "the global maximum".  token_in == token_out is allowed: the best
 * cycle through that token.
 *   amount_out, n_hops, status   [count]
 *   hop_seg, hop_row, hop_coin_in, hop_coin_out   [max_hops][count], hop-major: exactly what cfmm_quote_path and cfmm_swap_path
 *                 take (with n_hops and max_hops); -1 in the slots at k >= n_hops[q]
 *   status[q]:
 *     CFMM_FOUND          a walk was found; every pool on it is visited once
 *     CFMM_FOUND_NONE     token_out is not reached within max_hops, or amount_in is 0: amount_out 0.0, n_hops 0, hop slots -1
 *     CFMM_FOUND_REPEATS  a walk was found and its amounts are cfmm_quote_path's, but it visits some pool more than once:
 *                         cfmm_swap_path would refuse it as one path
 * Everything is checked before anything is enqueued: count >= 0, max_hops, no null array, every token in 0 .. n_tokens-1, every
 * amount finite and >= 0.  A failure is CFMM_ERR_INVALID_ARG, names the query ("cfmm_find_path: query 12: ...") and leaves the
 * outputs untouched.  Read-only exactly as cfmm_quote: no state moves, no earlier trades or outputs are invalidated.
 * Synchronous on the context's stream; count == 0 is a no-op; a context without pools answers CFMM_FOUND_NONE everywhere;
 * large-market mode needs nothing special.  A MULTI-DEVICE CONTEXT answers CFMM_ERR_UNSUPPORTED.  One launch per layer with one
 * lane per pool, then one sparse launch per layer walking back; the scratch, (max_hops + 1) x queries x n_tokens x 8 bytes, is
 * kept by the context and bounded by 256 MiB: a larger call is processed in chunks of queries, with the same results.
 * Read-only options under "time_kernels": "find_relax_ns" and "find_walk_ns", the sums of the latest call's layer launches
 * and walk-back launches ("find_relax_ns_<h>", "find_claim_ns_<h>", "find_advance_ns_<h>", h = 1 .. 8: the same layer by
 * layer); "find_launches", all kernel launches of the latest call.  Option "find_lds" (default 1): the layer launches fold
 * their candidates through a per-block LDS copy of the layer rows where n_tokens lets one fit; 0 sends every candidate to
 * global memory -- the same bits, a measurement switch. */
#define CFMM_FOUND 0
#define CFMM_FOUND_NONE 1
#define CFMM_FOUND_REPEATS 2
int cfmm_find_path(cfmm_ctx* ctx, int64_t count, int32_t max_hops, const int32_t* token_in, const int32_t* token_out,
                   const double* amount_in, double* amount_out, int32_t* n_hops, int32_t* hop_seg, int64_t* hop_row,
                   int32_t* hop_coin_in, int32_t* hop_coin_out, int32_t* status);

/* netflows!(psi, r) -- src/router.jl:111-119, for the most recent sweep. */
int cfmm_netflows(cfmm_ctx* ctx, double* psi);
/* the `acc` of fn (src/router.jl:79-83) for the most recent sweep. */
int cfmm_dual_value(cfmm_ctx* ctx, double* acc);

/* ---- device-resident variants (stream / RCCL interop; no host round trip) -------------- */

/* d_v: n_tokens device doubles (must be finite and > 0, src/cfmms.jl:129: the library cannot validate device
 * memory; non-positive prices give undefined trades).  The library cannot see these prices, so with "fast_math" (default)
 * the launch carries BOTH arithmetics and every block picks from the prices it stages: inside [2^-150, 2^150] the fast
 * one, anything else -- NaN included -- the compiler's full-range sequences, under which a NaN price propagates into the
 * trades and psi of every pool that touches the token exactly as the reference's arithmetic does.  The call never refuses
 * and never changes the context's state.  (Round 4 launched the fast kernels on trust and reported a refusal on a LATER
 * call; host-pointer calls and cfmm_route choose the kernel per call, from the prices they are given.)
 * d_out: n_tokens+1 device doubles = {psi..., acc}: the
 * buffer a sharded run all-reduces (one collective per evaluation).  Asynchronous on the
 * context's stream.  materialize != 0: also write Delta/Lambda (find_arb! semantics). */
int cfmm_sweep_dev(cfmm_ctx* ctx, const double* d_v, double* d_out, int materialize);
/* Device addresses of the trade rows of the latest materialising sweep ([m_total][2] doubles each, the
 * reference's Delta / Lambda layout), valid until pools change.  With "compact_trades" (default) these
 * are expanded copies written on the context's stream by this call: call it again after a later sweep. */
/* Markets with weighted or Curve pools: CFMM_ERR_UNSUPPORTED (their trades are ragged and stay per segment; cfmm_get_trades). */
int cfmm_trades_dev(cfmm_ctx* ctx, const double** d_delta, const double** d_lambda);

/* With option "time_kernels"=1 every sweep launch is bracketed by hipEvents on the launch
 * stream.  Returns and resets: number of timed sweep-kernel launches, their summed
 * duration, and the same for the partial-reduction kernel. */
int cfmm_kernel_times(cfmm_ctx* ctx, int64_t* sweep_launches, double* sweep_ms,
                      int64_t* reduce_launches, double* reduce_ms);

/* ---- sharded runs: the all-reduce of {psi, acc} over xGMI peer mappings, inside the fold launch -- */

/* Sharded operation of a context (one process per GPU): after this call EVERY sweep of the context --
 * cfmm_find_arb, cfmm_eval, cfmm_route, and cfmm_sweep_dev -- returns the psi / acc of the WHOLE
 * market while the context stores only this rank's shard: the launch that folds the partial rows
 * also performs the all-reduce over the given symmetric buffers (block b publishes its columns as
 * self-validating 8-byte granules {sequence tag, 32 payload bits} in this rank's buffer -- no flag, no
 * fence -- and adds the same columns of every peer in rank order: every rank obtains bit-identical
 * results).  Buffer layout, per rank, with count = n_tokens + 1, zero-initialised before first use:
 *     [2][count][2] uint64 granules  =  cfmm_peer_buffer_bytes(n_tokens) bytes
 * (peer_buffers[p] = address of rank p's buffer mapped into THIS process; cfmm_peer_buffer_alloc / _open below, or any
 * other symmetric allocation).  It replaces nothing in the reference (which has no distributed path): it is the
 * collective of SURVEY 8e.  Every rank
 * must issue the same sequence of sweeps (route! does: all ranks take bit-identical L-BFGS-B steps).
 * seq = number of sharded sweeps already performed on these buffers (0 for fresh ones).  A rank
 * waits up to CFMM_AMD_PEER_TIMEOUT_S seconds (environment, default 30) for a peer, then the output
 * is NaN and host-pointer calls fail with CFMM_ERR_STATE.  world = 0 switches sharding off. */
int cfmm_set_peers(cfmm_ctx* ctx, const uint64_t* peer_buffers, int32_t world, int32_t rank, uint64_t seq);

/* The symmetric buffers of cfmm_set_peers without any framework: every rank allocates its buffer
 * (fine-grained device memory, sized and zeroed for the context's n_tokens), publishes the 64-byte IPC handle through whatever channel
 * its launcher has (MPI, torch.distributed, a file), and maps the other ranks' buffers from their handles
 * (hipIpcGetMemHandle / hipIpcOpenMemHandle; needs HSA_ENABLE_IPC_MODE_LEGACY=0 on this driver stack).
 * The pointers go to cfmm_set_peers (own rank: the pointer from _alloc).  _close unmaps a peer's buffer,
 * _free releases the own one (after every peer has closed it). */
#define CFMM_IPC_HANDLE_BYTES 64
int64_t cfmm_peer_buffer_bytes(int32_t n_tokens);
int cfmm_peer_buffer_alloc(cfmm_ctx* ctx, uint64_t* d_buf, unsigned char handle[CFMM_IPC_HANDLE_BYTES]);
int cfmm_peer_buffer_open(cfmm_ctx* ctx, const unsigned char handle[CFMM_IPC_HANDLE_BYTES], uint64_t* d_peer);
int cfmm_peer_buffer_close(cfmm_ctx* ctx, uint64_t d_peer);
int cfmm_peer_buffer_free(cfmm_ctx* ctx, uint64_t d_buf);

/* ---- sharded runs through RCCL: north_star's "RCCL all-reduce of psi and grad g over xGMI per outer iteration" ---- */

/* The same contract as cfmm_set_peers -- after the call EVERY sweep of the context (cfmm_find_arb, cfmm_eval, cfmm_route,
 * cfmm_sweep_dev) returns the psi / acc of the WHOLE market while the context stores this rank's shard of the axis the
 * reference threads over (src/router.jl:39) -- with the collective done by RCCL: behind every sweep's row fold the library
 * enqueues ncclAllReduce(d_out, d_out, n_tokens + 1, ncclDouble, ncclSum, comm, stream) on the context's stream (one
 * 4 KB collective per evaluation: latency, never link bandwidth).  No torch, no Python, no IPC handles: a Julia / C host
 * shards a market in three calls --
 *     rank 0:      cfmm_rccl_unique_id(id);          then broadcasts the 128 bytes with whatever its launcher has
 *     every rank:  cfmm_rccl_init_rank(ctx, id, world, rank);   (collective: returns when all ranks have joined)
 * -- or hands over a communicator it created itself (cfmm_set_rccl_comm: the caller keeps ownership; NULL switches the
 * exchange off).  RCCL sums in its own (ring / tree) order: every rank receives the SAME bits (the lockstep L-BFGS-B of
 * cfmm_route relies on it), but not the rank-ordered sum of cfmm_set_peers.  cfmm_set_peers (fold + exchange in ONE
 * launch: no second launch on the critical path of an evaluation) stays the fast path; this is the portable one
 * (cfmmrouter.jl_amd/dist.py tries the peer exchange first, then this, then torch.distributed).  One exchange at a time per context (CFMM_ERR_STATE otherwise);
 * evaluations are launched when their prices are ready (no pre-arming); n_tokens <= 8192.  RCCL is resolved at first use,
 * ALL entry points from ONE image: the one named by CFMM_AMD_RCCL_LIB (environment; path or soname), else the process's
 * global scope if ncclAllReduce is visible there, else librccl.so.1 -- CFMM_ERR_UNSUPPORTED if there is none.
 * cfmm_set_rccl_comm takes a foreign communicator only in the first two cases (the caller's own RCCL: a communicator must
 * meet the ncclAllReduce of the image that created it); cfmm_rccl_init_rank works in all three.
 * Failure semantics: RCCL's, not cfmm_set_peers'.  The all-reduce has NO time limit of its own -- a rank that fails before
 * it enqueues its ncclAllReduce (a launch error, an exception between two evaluations of a host-driven loop) leaves the
 * other ranks waiting in their stream synchronisation, exactly like any NCCL program; bound it with RCCL's own watchdog /
 * ncclCommAbort from the launcher, or use cfmm_set_peers, whose waits are bounded (CFMM_AMD_PEER_TIMEOUT_S).  A sweep whose
 * all-reduce could not be enqueued returns the error AFTER its local sweep and fold were launched: trades of a materialising
 * sweep exist, {psi, acc} do not (cfmm_netflows: CFMM_ERR_STATE). */
#define CFMM_RCCL_ID_BYTES 128
int cfmm_rccl_unique_id(unsigned char id[CFMM_RCCL_ID_BYTES]);
int cfmm_rccl_init_rank(cfmm_ctx* ctx, const unsigned char id[CFMM_RCCL_ID_BYTES], int32_t world, int32_t rank);
int cfmm_set_rccl_comm(cfmm_ctx* ctx, void* nccl_comm /* ncclComm_t, or NULL */);

/* ---- route! without an interpreter in the loop ----------------------- */

#define CFMM_OBJ_LINEAR_NONNEGATIVE 0 /* LinearNonnegative(c)      src/objectives.jl:51-79 */
#define CFMM_OBJ_BASKET_LIQUIDATION 1 /* BasketLiquidation(i, Din) src/objectives.jl:92-129 */

typedef struct cfmm_route_info {
    double f;            /* dual value g(v*) */
    double proj_grad;    /* max-norm of the projected gradient at v* */
    int32_t iterations;  /* L-BFGS-B iterations */
    int32_t evaluations; /* fn/g! evaluations == device sweeps inside the solver */
    int32_t sweeps;      /* all device sweeps incl. prologue and epilogue (src/router.jl:104,107) */
    int32_t status;      /* 0 pgtol, 1 factr, 2 maxiter, 3 maxfun, 4 line search, 5 non-finite f */
    double sweep_seconds;  /* wall time spent inside device sweeps (launch to results on the host), all sweeps */
    double total_seconds;  /* wall time of the whole call; the difference is the host-side L-BFGS-B */
} cfmm_route_info;

/* route!(r; v, m, factr, pgtol, maxfun, maxiter) -- src/router.jl:58-108, with the external
 * LBFGSB.jl solver (src/router.jl:60,105) replaced by this library's own L-BFGS-B
 * (csrc/lbfgsb.cpp, written from the published algorithm).  objective_vec is `c`
 * (LinearNonnegative) or `Din` (BasketLiquidation, objective_index = 0-based output token);
 * v0 may be NULL (the reference's default ones(n)/n, :62).  On return v_out[n] = r.v,
 * psi_out[n] = netflows(r), trades are materialised at v* (cfmm_get_trades).  Pass
 * maxfun = maxiter = 15000, m = 5, factr = 1e1, pgtol = 1e-5 for the reference's defaults. */
int cfmm_route(cfmm_ctx* ctx, int32_t objective_kind, const double* objective_vec, int32_t objective_index,
               const double* v0, int32_t m, double factr, double pgtol, int32_t maxfun, int32_t maxiter,
               double* v_out, double* psi_out, cfmm_route_info* info);

/* The solver alone on a caller-supplied objective (used by the CPU tests to compare it with
 * SciPy's L-BFGS-B).  nbd[i]: 0 free, 1 lower, 2 both, 3 upper.  fg returns f and fills g.
 * boxed_from_nbd != 0: like the Fortran code, treat the problem as "boxed" (unit first step) when
 * every nbd[i] == 2 even if a bound is infinite -- what the reference's call does
 * (src/router.jl:67-70) and what cfmm_route uses; 0: infinite bounds are no bounds (SciPy). */
typedef double (*cfmm_fg_callback)(void* user, const double* x, double* g);
int cfmm_lbfgsb_minimize(int32_t n, double* x, const double* lower, const double* upper, const int32_t* nbd,
                         cfmm_fg_callback fg, void* user, int32_t m, double factr, double pgtol, int32_t maxfun,
                         int32_t maxiter, int32_t boxed_from_nbd, cfmm_route_info* info);

/* Number of segments and their description (kind, pool count, launch geometry). */
int32_t cfmm_segment_count(const cfmm_ctx* ctx);
int cfmm_segment_info(const cfmm_ctx* ctx, int32_t seg, int32_t* kind, int64_t* m, int32_t* block,
                      int32_t* grid);

/* ==== EXPERIMENTAL -- beyond the reference's verbs ====================================================================
 * Everything ABOVE this line is the drop-in surface: the reference's own verbs (Router, find_arb!, route!, netflows,
 * update_reserves!, the objectives) and what sharding them needs.  What follows is NOT in CFMMRouter.jl, may change, and
 * is not needed to replace the reference's path:
 *   - cfmm_polish (below),
 *   - the option "stop_in_noise" (cfmm_set_option; default 0 = the stopping rules of L-BFGS-B 3.0).
 * (Test hooks are not in this library: `make -C cfmmrouter.jl_amd/csrc hooks` builds libcfmm_amd_hooks.so with
 * -DCFMM_TEST_HOOKS for tests/test_gpu_armed.py.)
 * ====================================================================================================================== */

/* Tighten a route!'s result beyond what L-BFGS-B's stopping rules can (NOT part of the reference: its route! ends where
 * LBFGSB.jl ends, src/router.jl:105-107).  L-BFGS-B's line search compares dual VALUES, whose rounding noise -- a sum
 * over all pools -- hides decreases below ~1e-15 relative; on interior optima that leaves a stationarity residual of
 * ~1e-6 max|psi|, on the reference's side as well.  cfmm_polish continues from v (in: a route!'s v*, out: the polished
 * point) with a projected chord-Newton iteration on the optimality conditions of the dual problem of src/router.jl:58-108,
 *     G_j(v) = 0 for l_j < v_j,   G_j(v) >= 0 for v_j = l_j,   G = grad f(objective, v) + psi(v),  l = lower_limit(objective),
 * using GRADIENTS only: J = forward-difference Jacobian of G at the start (n_tokens + 1 fused sweeps, step rel_step * v_j;
 * pass rel_step <= 0 for 1e-7), free set F = {j : not (v_j = l_j and G_j > 0)}, v_F <- max(l_F, v_F - J_FF^-1 G_F); steps that
 * do not reduce the residual are halved, the best iterate is kept, at most max_iters iterations (8 is plenty).  Ends with
 * find_arb!(r, v) like route! does: psi_out[n] = netflows(r), trades materialised at the polished point.  Objective
 * arguments as for cfmm_route.  The Python mirror's polish_ (cfmmrouter.jl_amd/router.py) is the same iteration.  Works on
 * multi-device contexts; on a cfmm_set_peers context every rank must make the same call (its sweeps are collective, and
 * all ranks see bit-identical psi, hence take identical steps). */
typedef struct cfmm_polish_info {
    double residual0;    /* max |G_F| before (and -G_j where a variable on its bound has G_j < 0) */
    double residual;     /* ... after */
    int32_t iterations;
    int32_t sweeps;      /* device sweeps of the call, Jacobian and final find_arb! included */
    double total_seconds;
} cfmm_polish_info;
int cfmm_polish(cfmm_ctx* ctx, int32_t objective_kind, const double* objective_vec, int32_t objective_index,
                double* v, int32_t max_iters, double rel_step, double* psi_out, cfmm_polish_info* info);

#ifdef __cplusplus
}
#endif
#endif
