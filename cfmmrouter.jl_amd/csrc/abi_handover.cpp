// abi_handover.cpp -- how an evaluation's result crosses to the host: host-pointer sweeps (cfmm_find_arb / cfmm_eval)
// through the zero-copy stage and its output granules, and the pre-armed evaluations cfmm_route uses -- signalled,
// cancelled and retried.  (How one evaluation is launched: abi_sweep.cpp.)
//   find_arb!(r, v)          src/router.jl:38-42     -> enqueue_sweep(materialize = true)
//   fn / g! per evaluation   src/router.jl:73-102    -> enqueue_sweep(materialize = false): {Ψ, acc}
//   netflows(r)              src/router.jl:111-125   -> cfmm_netflows (the Ψ of the latest sweep)
#include "ctx.h"
#include "granule.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>

using namespace cfmm;

namespace cfmm {

int check_prices(cfmm_ctx* c, const double* v)
{
    if (!v) return fail(c, CFMM_ERR_INVALID_ARG, "v is null");
    for (int j = 0; j < c->n; ++j)
        if (!(v[j] > 0.0) || !std::isfinite(v[j]))
            return fail(c, CFMM_ERR_INVALID_ARG, "v[%d] must be finite and > 0 (src/cfmms.jl:129)", j);
    return CFMM_OK;
}

// every price in [2^-kFastExp, 2^kFastExp] (sweep.h): the host's half of the fast kernels' precondition
bool prices_in_fast_window(const double* v, int n)
{
    for (int j = 0; j < n; ++j) {
        uint64_t bits;
        std::memcpy(&bits, v + j, sizeof bits);
        const int e = (int)((bits >> 52) & 0x7ff);
        if (e < 1023 - kFastExp || e > 1023 + kFastExp) return false;
    }
    return true;
}

// Why did a sweep deliver NaN?  The blocks report through the sticky word (sweep.h kFlagWindow / kFlagGaveUp).
// Returns the reported bits among `mask` and clears exactly those (a report nobody asked about stays for whoever does).
unsigned long long HostStage::take_flags(unsigned long long mask)
{
    if (!buf) return 0;
    // atomic on the mapped word: launches queued behind the current one may report (system-scope fetch_or over PCIe) while the
    // host clears -- a plain read-modify-write could lose their bit
    unsigned long long* w = reinterpret_cast<unsigned long long*>(buf.host() + flag_off);
    if ((__atomic_load_n(w, __ATOMIC_ACQUIRE) & mask) == 0) return 0;
    return __atomic_fetch_and(w, ~mask, __ATOMIC_ACQ_REL) & mask;
}

// First half of a host-pointer sweep: stage v, enqueue the evaluation (asynchronous).
int host_sweep_begin(cfmm_ctx* c, const double* v, bool materialize)
{
    HIP_TRY(c, hipSetDevice(c->device));
    (void)c->stage.take_flags(kFlagWindow);     // a stale report must not label a later overflow of THIS call
    std::memcpy(c->stage.buf.host(), v, (size_t)c->n * sizeof(double));
    if (materialize) {
        c->trade_v.assign(v, v + c->n);   // the prices the device trades belong to (update_reserves!)
        // find_arb!(r, v) is a function of v alone (test/arb.jl:16 compares its netflows exactly): a materialising host call
        // always walks forwards, whatever ran before; the alternation (option "alternate") restarts behind it.
        c->sweep_count = 0;
    }
    const bool zero_copy = c->opt_zero_copy != 0 && c->stage.buf.dev() != nullptr;
    // v: small vectors are read by every block straight from the mapped pinned buffer (the PCIe
    // round trip hides behind the first tile's pool loads); larger ones go through one H2D copy.
    const double* v_src = c->stage.buf.dev();
    if (!zero_copy || c->n > 1024 || global_bins(c)) {
        HIP_TRY(c, hipMemcpyAsync(c->d_v.get(), c->stage.buf.host(), (size_t)c->n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        v_src = c->d_v.get();
    }
    // {Ψ, acc}: as output granules in the mapped pinned buffer when it can (polled by host_sweep_end), else d_out + a copy
    const bool want_host_out = zero_copy && c->opt_host_flag != 0;
    int rc = enqueue_sweep(c, v_src, c->d_out.get(), materialize, want_host_out, 0,
                           prices_in_fast_window(v, c->n) ? kPricesInWindow : kPricesOutside);
    if (rc != CFMM_OK) return rc;
    if (!c->stage.last_host_out)
        HIP_TRY(c, hipMemcpyAsync(c->stage.out(), c->d_out.get(), (size_t)(c->n + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return CFMM_OK;
}

// Output granules of the sweep with sequence number `seq` (fold_finish; granule.h): true once all 2(n+1) carry its tag;
// the doubles are then reassembled into the {Ψ, acc} slots of the staging buffer.
bool HostStage::granules_arrived(uint64_t seq)
{
    const unsigned long long tag = granule_tag(seq);
    const volatile unsigned long long* g = reinterpret_cast<const volatile unsigned long long*>(buf.host() + gran_off);
    const int n1 = n + 1;
    if ((g[2 * n1 - 1] >> 32) != tag || (g[0] >> 32) != tag) return false;   // cheap rejects: last and first granule
    double* h_out = out();
    for (int j = 0; j < n1; ++j)
        if (!granule_join(g[2 * j], g[2 * j + 1], tag, h_out[j])) return false;
    return true;
}

// Poll for those granules instead of waiting for the kernel's end-of-pipe processing and its completion signal: at most
// max_spins polls and -- limit_s > 0 -- about that many seconds (the clock is read every 65536 polls).  True: they are here.
bool HostStage::wait(uint64_t seq, long max_spins, double limit_s)
{
    bool seen = false;
    const auto t0 = limit_s > 0 ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    for (long spins = 0; spins < max_spins; ++spins) {
        if (granules_arrived(seq)) { seen = true; break; }
        __builtin_ia32_pause();
        if ((spins & 0xffff) == 0xffff && limit_s > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
            break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return seen;
}

namespace {

// {Ψ, acc} have arrived in the pinned staging buffer: take them over into last_out.
int take_host_out(cfmm_ctx* c)
{
    const double* h_out = c->stage.out();
    c->last_out.assign(h_out, h_out + c->n + 1);
    for (int j = 0; j <= c->n; ++j)
        if (!std::isfinite(c->last_out[(size_t)j])) {
            c->have_out = false;
            (void)hipStreamSynchronize(c->stream);
            const unsigned long long why = c->stage.take_flags(kFlagWindow);
            if (why & kFlagWindow)     // (a fast kernel met prices the host had vouched for: cannot happen unless v changed under the call)
                return fail(c, CFMM_ERR_STATE, "non-finite {psi, acc}: a price lies outside the window of the fast arithmetic "
                                               "(the price vector changed while the call ran?)");
            if (c->rccl_comm)
                return fail(c, CFMM_ERR_STATE, "non-finite {psi, acc}[%d] after the RCCL all-reduce: a shard overflowed (on some rank)", j);
            if (!c->peers.empty())
                return fail(c, CFMM_ERR_STATE, "non-finite {psi, acc}[%d]: the peer all-reduce timed out (a rank did not "
                                               "publish within CFMM_AMD_PEER_TIMEOUT_S) or a shard overflowed", j);
            return fail(c, CFMM_ERR_STATE, "non-finite {psi, acc}[%d]: pool arithmetic overflowed", j);
        }
    c->have_out = true;
    return CFMM_OK;
}

} // namespace

// Second half: wait for {Ψ, acc} to be on the host and take them over into last_out.
int host_sweep_end(cfmm_ctx* c)
{
    HostStage& st = c->stage;
    // the fold blocks wrote {Ψ, acc} as self-validating granules into the pinned buffer: poll them.  Bounded; falls back to
    // a stream wait.
    if (!(st.last_host_out && st.wait(st.out_seq, 400000000L, 0.0))) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (st.last_host_out && !st.granules_arrived(st.out_seq)) {
            c->have_out = false;
            return fail(c, CFMM_ERR_STATE, "the sweep retired without delivering its outputs");
        }
    }
    return take_host_out(c);
}

int single_host_sweep(cfmm_ctx* c, const double* v, bool materialize)
{
    int rc = host_sweep_begin(c, v, materialize);
    return rc != CFMM_OK ? rc : host_sweep_end(c);
}

int host_sweep(cfmm_ctx* c, const double* v, bool materialize)
{
    int rc = check_prices(c, v);
    if (rc != CFMM_OK) return rc;
    return c->shards.empty() ? single_host_sweep(c, v, materialize) : multi_host_sweep(c, v, materialize);
}

// ---- pre-armed evaluations (cfmm_route; sweep.h SweepArgs::arm_word) ---------------------------
// cfmm_route's evaluations are strictly sequential (the solver needs {Ψ, acc} of v_k to choose v_k+1), so the ~5 us
// between "v is ready" and "the kernel's first wavefront runs" (launch call, doorbell, command processor, dispatch)
// sit on the critical path of every evaluation.  Armed operation takes them off it: evaluation k+1 -- sweep and
// fold -- is enqueued right after evaluation k has been signalled, becomes resident when k's fold retires, issues its
// first pool loads, clears its LDS bins and then polls a word in device memory; the host writes v_k+1 and the word
// straight into (fine-grained) device memory through the PCIe BAR.  Measured on the handoff alone
// (scripts/native/handoff.hip, profiles/r02_handoff.txt): 11.2 us launch-when-ready vs 6.3 us armed.
// The one launch left over when the solver stops is cancelled through the same word.
//
// Sharded contexts arm as well (round 3).  cfmm_set_peers: every rank arms its own launches; the ranks run the same
// solver on bit-identical {Ψ, acc}, so they signal and cancel the same evaluations, and a cancelled fold + gather
// publishes nothing (its sequence number is reused).  Multi-device parents: the calling thread writes v into every
// shard's BAR window, then polls every shard's output granules and sums them in device order -- no worker threads on
// this path.  NOT armed: parents whose shards share a device, and therefore the ranks-on-one-GPU test set-ups (they
// switch the option off): a polling launch occupies its CUs, and a shard of the SAME evaluation queued behind it on
// the same device would wait for an evaluation that waits for it.
void ArmState::write(const double* v, uint64_t word)
{
    if (v) std::memcpy(buf.get(), v, (size_t)n * sizeof(double));      // write-combining stores through the BAR
    __builtin_ia32_sfence();                                            // v before the word (WC buffers flush out of order)
    *reinterpret_cast<volatile unsigned long long*>(buf.get() + n_pad) = word;
    __builtin_ia32_sfence();                                            // and out now
}

namespace {

bool can_arm_single(cfmm_ctx* c)
{
    if (c->opt_armed == 0 || !c->arm.buf || c->opt_zero_copy == 0 || !c->stage.buf.dev() || c->opt_host_flag == 0 ||
        c->opt_time_kernels != 0 || c->n > 1024 || c->stream != c->own_stream.get() || global_bins(c) || c->rccl_comm != nullptr)
        return false;
    return ensure_geometry(c) == CFMM_OK && c->rows_total > 0;
}

int armed_enqueue(cfmm_ctx* c)
{
    const uint64_t seq = ++c->arm.seq;
    int rc = enqueue_sweep(c, c->arm.buf.get(), c->d_out.get(), false, true, seq);
    if (rc != CFMM_OK) return rc;
    c->arm.tag = c->stage.out_seq;
    c->arm.pending = true;
    return CFMM_OK;
}

void armed_cancel_single(cfmm_ctx* c)
{
    if (!c->arm.pending) return;
    c->arm.write(nullptr, c->arm.seq | kArmCancel);
    c->arm.pending = false;
    --c->sweep_count;   // the cancelled launch swept nothing: later sweeps keep the tile directions of an unarmed run
    if (!c->peers.empty()) --c->peer_seq;   // ... and the peers' sequence number is reused (every rank cancels the same launch)
}

// Signal the waiting launch (enqueuing it first if none is waiting) and enqueue the next one behind it.
// `signalled` = an evaluation is now running whose outputs carry the sequence number `want` (a failure after that point
// concerns the NEXT launch only).
int armed_signal(cfmm_ctx* c, const double* v, uint64_t& want, bool& signalled)
{
    signalled = false;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->arm.pending) {
        int rc = armed_enqueue(c);
        if (rc != CFMM_OK) return rc;
    }
    want = c->arm.tag;
    c->arm.write(v, c->arm.seq);
    c->arm.pending = false;
    signalled = true;
    return armed_enqueue(c);   // evaluation k+1 goes out while k runs
}

// The signalled evaluation is lost: cancel the launch queued behind it, drain the stream, and put the bookkeeping back
// to where an unarmed run would be (the lost launch swept nothing useful: the retry takes its tile direction).  On a
// cfmm_set_peers context a lost evaluation is fatal -- the other ranks have moved on with it.
void armed_lost(cfmm_ctx* c, bool& retry)
{
    armed_cancel_single(c);
    (void)hipStreamSynchronize(c->stream);
    c->have_out = false;
    retry = c->peers.empty();
    if (retry) --c->sweep_count;
}

// Wait for the signalled evaluation's granules.  CFMM_ERR_STATE with `lost` set: the device never delivered (host
// stalled past the arm timeout between two evaluations, or the device never saw the word): the caller may retry unarmed.
// The bound: the device-side wait of the launch (arm_timeout_ms; on cfmm_set_peers contexts at least the peer timeout,
// see enqueue_sweep) plus, on peers contexts, the time its fold + gather may legitimately wait for a slower rank.
int armed_wait(cfmm_ctx* c, uint64_t want, bool& lost)
{
    lost = false;
    const double arm_s = 1e-3 * (double)std::min<int64_t>(std::max<int64_t>(c->opt_arm_timeout_ms, 1), 10000);
    const double peer_s = 1e-8 * (double)c->peer_timeout_ticks;
    const double limit = c->peers.empty() ? 2.0 * arm_s + 1.0 : std::max(arm_s, peer_s) + peer_s + 2.0;
    if (!c->stage.wait(want, LONG_MAX, limit)) {
        armed_lost(c, lost);
        (void)c->stage.take_flags(kFlagGaveUp);
        return fail(c, CFMM_ERR_STATE, c->peers.empty()
                        ? "armed evaluation did not complete (the device never saw its price vector)"
                        : "armed evaluation did not complete within the arm + peer timeouts (this rank's launch never saw its "
                          "price vector, or a peer never published)");
    }
    // NaN in the dual column: the blocks say why through the sticky report word.  A launch that gave up waiting for its
    // prices is a LOST evaluation (retried unarmed by the caller); anything else -- arithmetic overflow, a peer gather that
    // timed out -- is reported by take_host_out as what it is.
    const double acc = c->stage.out()[c->n];
    if (acc != acc) {
        const unsigned long long why = c->stage.take_flags(kFlagGaveUp);
        if (why & kFlagGaveUp) {
            armed_lost(c, lost);
            return fail(c, CFMM_ERR_STATE, "armed evaluation gave up waiting for its price vector (host stalled longer than the arm timeout)");
        }
    }
    int rc = take_host_out(c);
    if (rc != CFMM_OK) armed_cancel_single(c);
    return rc;
}

} // namespace

bool can_arm(cfmm_ctx* c)
{
    if (!is_parent(c)) return can_arm_single(c);
    if (c->opt_armed == 0 || !c->shards_distinct) return false;
    for (cfmm_ctx* child : c->shards)
        if (!child->segs.empty() && !can_arm_single(child)) return false;
    return true;
}

void armed_cancel(cfmm_ctx* c)
{
    if (!c) return;
    if (!is_parent(c)) return armed_cancel_single(c);
    for (cfmm_ctx* child : c->shards) armed_cancel_single(child);
}

// One fused evaluation at v through the armed launches.  A lost evaluation (see armed_wait) is retried ONCE through the
// launch-when-ready path before the call fails: a host that was paused between two evaluations (debugger, SIGSTOP,
// oversubscription) costs a retry, not the route.  *lost_out tells the caller (cfmm_route stops arming for the rest of
// the call: whatever stalled the hand-over once -- e.g. another process's launches holding this GPU's CUs -- may do so again).
int armed_eval(cfmm_ctx* c, const double* v, bool* lost_out)
{
    if (lost_out) *lost_out = false;
    int rc = check_prices(c, v);
    if (rc != CFMM_OK) return rc;
    if (!prices_in_fast_window(v, c->n)) {
        // the waiting launch runs the fast arithmetic (its kernel was chosen before these prices existed): cancel it and
        // evaluate launch-when-ready on the full-range kernels; the caller stops arming (prices this extreme stay extreme)
        armed_cancel(c);
        if (lost_out) *lost_out = true;
        return is_parent(c) ? multi_host_sweep(c, v, false) : single_host_sweep(c, v, false);
    }
#ifdef CFMM_TEST_HOOKS
    if (c->opt_debug_stall_ms > 0 && c->arm.pending) {   // test hook: the host "stalls" once while a launch waits for its prices
        std::this_thread::sleep_for(std::chrono::milliseconds(c->opt_debug_stall_ms));
        c->opt_debug_stall_ms = 0;
    }
#endif
    if (!is_parent(c)) {
        uint64_t want = 0;
        bool signalled = false;
        const int rc_next = armed_signal(c, v, want, signalled);
        if (!signalled) return rc_next;
        bool lost = false;
        rc = armed_wait(c, want, lost);
        if (rc != CFMM_OK && lost) {
            armed_cancel_single(c);
            if (lost_out) *lost_out = true;
            return single_host_sweep(c, v, false);
        }
        if (rc != CFMM_OK) return rc;
        return rc_next;
    }
    const int nd = (int)c->shards.size();
    std::vector<uint64_t> want((size_t)nd, 0);
    std::vector<int> rcs((size_t)nd, CFMM_OK);
    std::vector<char> running((size_t)nd, 0);
    for (int d = 0; d < nd; ++d)
        if (!c->shards[(size_t)d]->segs.empty()) {
            bool signalled = false;
            rcs[(size_t)d] = armed_signal(c->shards[(size_t)d], v, want[(size_t)d], signalled);
            running[(size_t)d] = signalled ? 1 : 0;
        }
    bool any_lost = false;
    int first_err = CFMM_OK, err_shard = -1;
    for (int d = 0; d < nd; ++d) {
        cfmm_ctx* child = c->shards[(size_t)d];
        if (child->segs.empty()) continue;
        if (!running[(size_t)d]) {
            if (first_err == CFMM_OK) { first_err = rcs[(size_t)d]; err_shard = d; }
            continue;
        }
        bool lost = false;
        const int rw = armed_wait(child, want[(size_t)d], lost);
        any_lost = any_lost || lost;
        running[(size_t)d] = (rw == CFMM_OK && !lost) ? 2 : 1;   // 2: this shard delivered the evaluation
        const int r = rw != CFMM_OK ? rw : rcs[(size_t)d];
        if (r != CFMM_OK && first_err == CFMM_OK) { first_err = r; err_shard = d; }
    }
    if (any_lost) {
        armed_cancel(c);
        for (int d = 0; d < nd; ++d)   // shards that did deliver repeat the evaluation too: it takes the same tile direction
            if (running[(size_t)d] == 2) --c->shards[(size_t)d]->sweep_count;
        if (lost_out) *lost_out = true;
        return multi_host_sweep(c, v, false);
    }
    if (first_err != CFMM_OK) {
        armed_cancel(c);
        c->have_out = false;
        return fail(c, first_err, "shard %d: %s", err_shard, c->shards[(size_t)err_shard]->err.c_str());
    }
    c->last_out.assign((size_t)c->n + 1, 0.0);   // the all-reduce: shard order, on the host
    for (int d = 0; d < nd; ++d) {
        const cfmm_ctx* child = c->shards[(size_t)d];
        if (child->segs.empty()) continue;
        for (int j = 0; j <= c->n; ++j) c->last_out[(size_t)j] += child->last_out[(size_t)j];
    }
    c->have_out = true;
    c->have_trades = false;
    return CFMM_OK;
}

} // namespace cfmm

extern "C" {

int cfmm_find_arb(cfmm_ctx* c, const double* v)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    return host_sweep(c, v, true);
}

int cfmm_eval(cfmm_ctx* c, const double* v, double* psi_out, double* acc_out)
{
    if (!c) return CFMM_ERR_INVALID_ARG;
    int rc = host_sweep(c, v, false);
    if (rc != CFMM_OK) return rc;
    c->have_trades = false; // trades on the device no longer correspond to the latest v
    if (psi_out) std::memcpy(psi_out, c->last_out.data(), (size_t)c->n * sizeof(double));
    if (acc_out) *acc_out = c->last_out[(size_t)c->n];
    return CFMM_OK;
}

int cfmm_netflows(cfmm_ctx* c, double* psi)
{
    if (!c || !psi) return CFMM_ERR_INVALID_ARG;
    if (!c->have_out) return fail(c, CFMM_ERR_STATE, "no sweep has been run yet");
    std::memcpy(psi, c->last_out.data(), (size_t)c->n * sizeof(double));
    return CFMM_OK;
}

int cfmm_dual_value(cfmm_ctx* c, double* acc)
{
    if (!c || !acc) return CFMM_ERR_INVALID_ARG;
    if (!c->have_out) return fail(c, CFMM_ERR_STATE, "no sweep has been run yet");
    *acc = c->last_out[(size_t)c->n];
    return CFMM_OK;
}

} // extern "C"
